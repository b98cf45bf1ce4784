// mrt_device.h -- internal (not installed): the tuning table, and the per-device /
// per-stream state shared by mrt_upload.hip (the owner, upload, stream contexts),
// mrt_device.hip (launches) and mrt_refit.hip.  host_api.cpp, plain C++, sees the tuning table only.
//
// Memory: a DeviceState and each of its StreamCtx hold one DevOwner, the only code in csrc
// that allocates or frees device memory, pinned memory, events and streams.  What an owner
// made it frees when it dies; the typed pointer fields beside it are views for the kernels'
// arguments.  Scratch that grows goes through reserve(): one group of buffers, one drain rule.
#pragma once
#include "mrt_image.h"

namespace mrt {

// Tuning knobs (mrt_set_tuning / mrt_get_tuning, host_api.cpp): A/B switches for
// performance work.  The member values are the defaults.
struct Tuning {
    int fast_box = 1;        // hardware min/max box test when its precondition holds
    int primary_waves = 7;   // launch-bounds occupancy target of the primary kernel: 0 (none), 6, 7, 8
    // shade1_kernel (the two-launch one-light shading) runs at 5 waves: 96 VGPRs, -2.5% vs 6 (round 2)
    int sched = 2;           // TileSched mode 0..3 (2 measured fastest)
    int batch_tpw = 2;       // bucket batches: tiles per wave the launch's grid is sized for when the batch is
                             // smaller than the persistent grid (a 1/4 or 1/8 split share): 2 -- C3 share model
                             // 2.98 -> 3.17x at N = 4, 4.69 -> 4.74x at N = 8; 4: 3.99x at N = 8
                             // (profiles/r04_share_tpw_ab.txt)
    int wave_log = 0;        // 1: timing-only wave log on uninstrumented launches (diagnostics)
    int scalar_nodes = 7;    // scalar-cache fetch of wave-uniform nodes (bit 0) and triangles (bit 1); bit 2:
                             // octant-ordered box test for waves whose rays share an octant (box_test_oct)
    int shade1 = 1;          // specialised shade kernel for one point light and one path
    int wavefront = 1;       // general shading: gen / trace / resolve kernels instead of one fused kernel
    int shadow_sched = -1;   // shadow_kernel schedule: 0 grid-stride, 1 XCD bands, 2 bands + lane refill,
                             // -1 auto: refill for dome-light (incoherent) rays, else bands
    // shadow_kernel's launch-bounds occupancy target is 8 waves (C4 / C5 -5.5% against none)
    int primary_inst_waves = 5;   // primary kernel of special-leaf scenes: 1 (none), 5, 6 (r02: 6 beat 1 by 5% on C5;
                                  // r03: 5 = 6 within 0.3% with binned shadow rays, and 96 VGPRs spill less)
    // the resolve pass (kernel 2c) of dome-light scenes runs at 4 waves (D1 -4%, C5 -1.2 ms against none;
    // special-leaf scenes at 3, without scratch);
    // the direct-lighting adaptive kernel at 6 (unbounded it takes 256 VGPRs: A3 30.7 -> 12.8 ms)
    int adapt_refill = 32;   // adaptive_kernel pixel refill: idle lanes that trigger a dequeue (0: tiles; 32: A3 -13%)
    int chain_shadow_step = 0;   // instanced chain levels: shadow rays walk with anyhit_step_inst (deferred proxies)
    // chain_trace_kernel of plain scenes runs at 8 waves (P4 -17%, R3 -3.5% against none)
    int near_first = -1;     // any-hit walks take the nearest hit child first: 0 off, 1 on, -1 auto
                             // (auto: on in the chunked shadow kernel of plain scenes only -- C4 shade
                             // -12.6%; off in the refill one, C5 +4.5%, the instanced chunked one,
                             // C5 +15%, and the fused kernels, C3 +5%, A3 / R3 +2%)
    int chain_shadow_refill = 0;   // instanced chain levels: shadow rays on the lane-refill kernel (FS: 6% slower, profiles/r04_fs_chain_shadow_refill_ab.txt)
    int chain = 1;           // REC scenes: wavefront chain engine (mrt_chain.hip) instead of the fused kernel
    int chain_est = 1;       // chain levels sized by the entries earlier chunks needed (0: worst case, 3^ceil(k/2))
    int chain_est_pct = 125; //   headroom over the largest count per path seen, percent
    int chain_mb = 8192;     // chain scratch per stream (MB), at most 80% of the device's free memory; larger frames
                             // run in chunks of work items.  With estimated level capacities 8 GB costs G3 3% against
                             // 48 GB and R3 / P4 / FS nothing (profiles/r04_chain_mb_est_ab.txt)
    int fused = 1;           // one point light, one path: frame1_kernel (primary + shading in one launch)
    int walk_exit = 1;       // the walk loop of frame1_kernel / primary_kernel: 1 one exit (a stack overflow
                             // empties the stack and leaves at the pop test), 0 two (the overflow returns).
                             // One exit issues 19% fewer SALU per wave step (C3 -7%, C4 -6%); round 5's
                             // 12-16% loss on the bunny scenes was the frame latency of a few heavy
                             // top-row tiles with only 4 frames in flight (walk exit), gone
                             // with 8 hardware queues: one exit everywhere, no probe (round 6)
    int walk_latch = 1;      // frame1_kernel's camera-ray walk: 1 one latch (the popping lanes pick their next node
                             // by select in the same step), 0 nested (two latches: lanes that pop wait for the
                             // wave's longest descent).  Round-6 A/B (profiles/r06_walk_latch_ab.txt): one latch
                             // C2 -11%, C3L -4.4%, C3 +1.5%; config C3 runs 0 (miro/scenes.py)
    int lds_nodes = 0;       // frame1_kernel's LDS top-node walk (LN), 0 off / 1 on: with 4 frames in flight C2
                             // -4.1%, C3 +9%, C3L +11% (profiles/r05_lds_nodes_ab_*.txt); no probe separated them
                             // reliably (single-frame kernel times are equal on C2), so it is off unless asked for
    int frame1_waves = 7;    // frame1_kernel launch-bounds occupancy target: 1 (none), 5..8 (7: -0.9% per frame with
                             // 4 frames in flight, +0.8% single-frame latency; profiles/r03_c3_scalar_waves_ab.txt)
    int bin = -1;            // ray binning (mrt_bin.h) before tracing: bit 0 the wavefront shadow pass (kernel 2b),
                             // bit 1 the chain levels' closest-hit entries, bit 2 the chain levels' shadow rays;
                             // -1 auto (bin_mode): chain levels of path-traced scenes (P4 -18% frame; the
                             // coherent mirror / glass levels of R3 / G3 lose their pixel order: +22% / +44%)
                             // and the dome shadow rays of instanced scenes, in the frame shadow pass (C5 -2.6%;
                             // D1 +2%) and in the chain levels (FS -29% per frame, profiles/r04_fs_bin_ab.txt),
                             // and the chain levels' shadow rays of dispersive scenes, whose three refraction
                             // children per split diverge (G3 -5% with 4 frames in flight; R3's coherent
                             // mirror levels +7%: off; profiles/r04_g3_bin_ab.txt)
    int chain_bands = -1;    // chain_trace_kernel: XCD-banded chunk queue (binned rays: one XCD's L2 holds its share);
                             // -1 auto: on when the level is binned (P4 -3.4%; unbinned R3 +5.7%, G3 +3%)
    int dome_replay = 1;     // dome-light resolve (2c) sums 2a's recorded samples instead of sampling again
    int bin_inst = 0;        // off: C5 shade pass +0.8% (profiles/r04_c5_bin_inst_primary_waves_ab.txt); instanced scenes' shadow-ray bins: instance-major keys (the ray's origin instance, BLAS-major)
    int bin_dbits = 2;       // binning key: direction cells per octahedral axis = 2^dbits
    int bin_obits = 2;       //   origin cells per scene-box axis = 2^obits (2 dbits + 3 obits <= 12);
                             //   sweep of 12 pairs: (2, 2) best on P4 (-18%) and C5 (-2.6%), finer
                             //   direction cells lose (P4 (6, 0) -11%), profiles/r03_bin_sweep.txt
};
extern Tuning g_tune;   // defined in host_api.cpp

}  // namespace mrt

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include <atomic>
#include <initializer_list>
#include <mutex>

namespace mrt {

#define HIP_OK(expr)                                                                    \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess) {                                                         \
            set_error(std::string(#expr) + ": " + hipGetErrorString(e_));               \
            return MRT_ERR_HIP;                                                         \
        }                                                                               \
    } while (0)

// ------------------------------------------------------------------ ownership
// Records what it creates and frees it in free_all / its destructor: events and streams
// first, then memory.  On failure the out-parameter stays as it was (null) and the HIP error
// text is set (MRT_ERR_HIP).  The current device is the owner's whenever it is used.
class DevOwner {
public:
    DevOwner() = default;
    DevOwner(const DevOwner&) = delete;
    DevOwner& operator=(const DevOwner&) = delete;
    ~DevOwner() { free_all(); }
    template <typename T> int alloc(T*& p, size_t bytes, bool pinned = false) {
        void* q = nullptr;
        const int rc = memory(q, bytes, pinned);
        if (q) p = static_cast<T*>(q);
        return rc;
    }
    template <typename T> int pinned(T*& p, size_t bytes) { return alloc(p, bytes, true); }
    int event(hipEvent_t& ev, unsigned flags = hipEventDefault);
    int stream(hipStream_t& st);   // non-blocking
    // allocate (16 bytes for an empty array) and copy from the host, synchronously
    template <typename T> int upload(T*& p, const void* src, size_t bytes) {
        void* q = nullptr;
        if (const int rc = alloc(q, bytes ? bytes : 16)) return rc;
        p = static_cast<T*>(q);
        if (bytes) HIP_OK(hipMemcpy(q, src, bytes, hipMemcpyHostToDevice));
        return MRT_OK;
    }
    void release(void* p);    // frees one recorded allocation and forgets it (null: nothing)
    void free_all();
    static int64_t live();    // what every owner of this process holds now (mrt_debug_live_resources)
private:
    struct Held { void* h; void (*destroy)(void*); bool memory; };
    int memory(void*& p, size_t bytes, bool pinned);
    void keep(void* h, void (*destroy)(void*), bool memory);
    std::vector<Held> held;
};

// A group of scratch buffers that share capacity fields: grown, never shrunk.  When a capacity
// falls short and a buffer of the group is live, `drain` (the stream whose launches may still
// read it; nullptr: none) is synchronised; then the whole group is released and allocated
// anew.  After a failed allocation the capacities stay 0, so the next call tries again.
struct GrowBuf { void** ptr; size_t bytes; };
struct GrowCap { size_t* cap; size_t need; };
int reserve(DevOwner& own, const hipStream_t* drain, std::initializer_list<GrowBuf> bufs, std::initializer_list<GrowCap> caps);

// ------------------------------------------------------------------ device state
// Launch scratch of one stream: everything a render / trace launch writes
// besides the caller's outputs.  Two launches on different streams never share
// one, so frames can overlap (the tail of one persistent launch with the start
// of the next).
struct StreamCtx {
    DevOwner own;                            // its buffers and events
    hipStream_t stream = nullptr;            // the caller's
    int32_t* gstack = nullptr;               // traversal-stack spill columns
    unsigned long long* ctr = nullptr;       // statistics + tile counters
    unsigned long long* wave_log = nullptr;  // 2 launches x grid x 4 waves x kLogWords u64 (diagnostics)
    int log_waves[2] = {0, 0};               // waves of the last logged primary / shade launch
    float4* hitbuf = nullptr;                // kernel 1 -> kernel 2 hand-off (per output slot)
    size_t hit_slots = 0;
    float4* rays = nullptr;                  // wavefront shadow rays: origin+tMax | direction
    uint8_t* occl = nullptr;                 // per ray: occluded
    uint8_t* nrays = nullptr;                // per output slot: rays written
    size_t ray_cap = 0, nrays_cap = 0;
    float* lvl = nullptr;                    // REC kernels: chain level records (RenderParams::lvl)
    size_t lvl_cap = 0;                      //   floats
    void* chain = nullptr;                   // wavefront chain engine scratch (mrt_chain.hip)
    size_t chain_bytes = 0;
    uint64_t chain_budget = 0;               // the chunk budget of its last chain-engine frame (bytes)
    uint32_t chain_chunks = 0;               //   and the chunks that frame ran
    void* adapt = nullptr;                   // chain-engine adaptive supersampling: means, pixel lists, unit colours
    size_t adapt_bytes = 0;
    // chain level capacities: per pass index (adapt_n, 0 = no supersampling) and level, the
    // largest entries per path a chunk on this stream needed (x 65536, + 1; 0 = not seen,
    // all ones = unknown) -- on the device (atomicMax by chain_merge), its last copy on the
    // host (pinned, in flight until est_ev), and the host's view used to size chunks
    uint32_t* est_dev = nullptr;
    uint32_t* est_pinned = nullptr;
    hipEvent_t est_ev = nullptr;
    bool est_pending = false;
    std::vector<uint32_t> est;
    bool last_was_render = false;
    bool fused = false;                      // the last render ran frame1_kernel (one launch)
    bool chain_used = false;                 // the last render's shading ran the wavefront chain engine
    bool supplied = false;                   // the last launch took the caller's hit records (CTR_INVALID is its count)
    uint16_t* bin_keys = nullptr;            // ray binning (mrt_bin.h): per-ray keys, two permutations
    uint32_t* bin_perm = nullptr;            //   [2][bin_cap] (0: shadow rays, 1: chain closest-hit entries)
    uint32_t* bin_hist = nullptr;            //   [2][kBinHist] bins + valid count
    size_t bin_cap = 0;
    float4* ray_e = nullptr;                 // dome-light replay (RenderParams::ray_e / lrec)
    uint32_t* lrec = nullptr;
    size_t ray_e_cap = 0, lrec_cap = 0;
    float* ls_aux = nullptr;                 // mrt_light_samples: per sample row, its factor of the specular sum
    int32_t* ls_counts = nullptr;            //   per (point, light): samples taken, where the caller asks for none
    size_t ls_aux_cap = 0, ls_counts_cap = 0;
    void* ls_rec = nullptr;                  //   the records (mrt_light_sample), where the caller asks for none
    size_t ls_rec_cap = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, evm = nullptr;
};
static constexpr int kMaxStreamCtx = 16;

// persistent buffers of one bucket share of mrt_render over several devices (owned by the replica)
struct ShareBuf {
    int32_t* items = nullptr;
    float* tiles = nullptr;
    size_t items_cap = 0, tiles_cap = 0;
    hipEvent_t done = nullptr;   // the share's tiles are in the caller's gather buffer
};

// Runs of PrimShade records that are consecutive triangles of one mesh (world objects in
// scene order, then every BLAS's): record start + k is triangle tri0 + k * step of `mesh`
// (mrt_hit_surfaces: HitInfo::obj of a hit on the device).
struct SurfaceGroup { int32_t start, mesh, tri0, step; };

struct DeviceState : ImageInfo {
    DevOwner own;                // every device array, scratch buffer, event and stream below but the contexts'
    int device = -1;
    SurfaceGroup* sgroups = nullptr;   // built by the first mrt_hit_surfaces call on this replica
    int n_sgroups = 0;
    QNode* nodes = nullptr;
    DLeaf* leaves = nullptr;
    PrimShade* prims = nullptr;
    float4* verts = nullptr;
    float4* normals = nullptr;
    DevMaterial* mats = nullptr;
    DevLight* lights = nullptr;
    DevDome* domes = nullptr;
    DevInstance* insts = nullptr;
    int32_t* inst_hit_base = nullptr;   // per instance: hit_base (ascending), for the instance-major bin keys
    uint16_t* inst_class = nullptr;     //   and its 7-bit class (BLAS-major rank)
    float4* inst_cell = nullptr;        //   object-space bin cells: BLAS box lo + BLAS bit, 4 / extent (2 per instance)
    DevTexture* texs = nullptr;   // material-map textures
    uint4* puv = nullptr;         // per prim texture-coordinate indices (nullptr: no texture-mapped mesh)
    float2* uvs = nullptr;
    float4* tans = nullptr;       // per normal: tangent / bitangent (texture-mapped meshes)
    float4* btans = nullptr;
    uint8_t* pflags = nullptr;    // motion blur: per world prim bit 0 = MBObject lane
    float4* verts2 = nullptr;     //   time-1 vertices parallel to verts (copies of verts for static meshes)
    const float* env = nullptr;  // environment texture
    uint16_t* tables = nullptr;
    uint8_t* gamma = nullptr;
    float* gammaF = nullptr;
    uint32_t gthreads = 0;
    // scratch for the synchronous API
    float* d_rgb = nullptr;
    uint8_t* d_rgb8 = nullptr;
    size_t frame_px = 0;
    int grid = 0;                // upper bound of any launch (kMaxBlocksPerCU per CU)
    std::atomic<int> lds_pick{-1};   // the last one-light frame ran the LDS top-node walk: 1 yes, 0 no, -1 none yet
    // refit (mrt_refit.hip), made by the first refit on this replica
    bool refit_ready = false;
    int32_t* refit_order = nullptr;       // device node numbers of the world, then of every BLAS, each sorted by height
    float4* refit_lbox = nullptr;         // per packet, world then BLASes, by device packet number: box min xyz, max xyz (2 float4)
    float4* refit_fixed = nullptr;        // ProxyObject lanes' boxes by instance, then MBObject lanes' (2 float4 each)
    int32_t* refit_mbslot = nullptr;      //   per world prim: its MBObject box after the instances', -1 = none
    float* refit_inst_m = nullptr;        // per instance: m_transform, 16 floats (refit_instance_kernel keeps it current)
    float* refit_stage = nullptr;         // the synchronous entry's packed vertices / normals on the device
    size_t refit_stage_cap = 0;           //   floats
    hipEvent_t refit_ev0 = nullptr, refit_ev1 = nullptr;
    int32_t* refit_blas_insts = nullptr;   // instance ids grouped by BLAS
    std::vector<int32_t> mesh_prim0;       // per mesh: its first world prim (its triangles follow in order), -1 = none
    // rebuild (mrt_rebuild.hip): what the first rebuild on this replica makes.  Dense node j of a
    // rebuilt world tree is device node j below rb_world_nodes (the world's node range of the
    // upload) and node rb_tail + (j - rb_world_nodes) above it: rb_extra nodes past the image's.
    bool rebuild_ready = false;
    bool sched_stale = false;             // the world's topology changed: the next refit makes refit_order again
    uint32_t rb_world_nodes = 0, rb_tail = 0, rb_extra = 0;
    uint32_t rb_cap_leaves = 0;           // packets of the world's range at the upload (the rebuilt tree uses the first P)
    uint32_t rb_cur_leaves = 0;           //   and those in use now
    uint64_t* rb_keys = nullptr;          // [2][4 rb_cap_leaves]: lane keys, unsorted and sorted
    float4* rb_lane_box = nullptr;        // per lane of the range: its box (2 float4)
    DLeaf* rb_leaves = nullptr;           // the P new packets before they are copied over the range
    float4* rb_seg = nullptr;             // min / max segment tree over the packet boxes: 2 P boxes, packet p at P + p
    uint64_t* rb_pkey = nullptr;          // per packet: the key of its first lane
    uint32_t* rb_pword = nullptr;         //   and the low four bits of its child word (count - 1, proxy, check)
    int32_t* rb_bin = nullptr;            // [4][P - 1]: first, last, left, right of the binary nodes
    uint32_t* rb_flag = nullptr;          // [2][P - 1]: roots a 4-wide node; its dense number (exclusive scan)
    uint32_t* rb_count = nullptr;         // the node count of the last rebuild
    void* rb_temp = nullptr;              // rocPRIM's scratch for the sort and the scan
    size_t rb_temp_bytes = 0;
    // relight (mrt_relight.hip): the records upload_scene wrote to domes / texs (their device
    // pointers), and what the first texture update on this replica makes
    std::vector<DevDome> dome_recs;
    std::vector<DevTexture> tex_recs;
    bool relight_ready = false;
    std::vector<float*> relight_sin;      // per dome: sin(theta) of its nv rows (dome_sin_theta)
    std::vector<float*> relight_int;      // per dome: int_v[nu], then int_u (what mrt_scene_dome_export adds to the tables)
    float* relight_tab = nullptr;         // scratch tables of one dome build, sized by the largest dome
    size_t relight_tab_cap = 0;           //   floats
    uint32_t* relight_status = nullptr;   // word 0: rejected async updates since the last status call; word 1: the last build passed
    float* relight_stage = nullptr;       // the synchronous entry's texels on the device
    size_t relight_stage_cap = 0;         //   floats
    hipEvent_t relight_ev0 = nullptr, relight_ev1 = nullptr;
    int cus = 0;
    int wall_khz = 0;            // wall_clock64() rate
    // per-stream launch scratch: frames on different streams are in flight at once
    std::mutex mu;
    std::vector<StreamCtx*> ctxs;
    StreamCtx* last = nullptr;   // context of the most recent launch (stats, wave log)
    std::vector<hipStream_t> share_streams;  // mrt_render over several devices: one stream per bucket share
    std::vector<ShareBuf*> share_bufs;       //   and its persistent item / tile buffers (+ copy-done event)
    hipStream_t gather_stream = nullptr;     //   the caller's device: frame assembly stream,
    float* g_tiles = nullptr;                //   every share's tiles gathered here,
    int32_t* g_items = nullptr;              //   their bucket ids
    size_t g_tiles_cap = 0, g_items_cap = 0;
};

// mrt_upload.hip
void free_replicas(Scene& s);
int get_ctx(DeviceState& d, hipStream_t stream, StreamCtx*& out);   // scratch context of `stream`
int ensure_device(Scene& s, int device);                            // the scene's replica on `device` becomes s.dev
// mrt_relight.hip: the texels of Scene::host_tex_stale and the DomeTables of host_dome_stale from
// replica d (sync_host's part for texture updates; the caller has synchronised the device)
int relight_read_back(Scene& s, DeviceState& d);
// mrt_refit.hip: what a refit of replica d needs beyond the upload (the current device is d's);
// after a rebuild (sched_stale) the height schedule alone, made again
int refit_prepare(const Scene& s, DeviceState& d);
// mrt_rebuild.hip: the world's topology, packets and boxes from replica d after a device
// rebuild, in canonical numbers (sync_host's part; the caller has synchronised the device)
int rebuild_read_back(Scene& s, DeviceState& d);

}  // namespace mrt
#endif   // __HIPCC__
