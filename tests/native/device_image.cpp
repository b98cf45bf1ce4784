// The host image of a device replica (build_image, csrc/host_image.cpp) on three scenes, without
// a GPU: the invariants every kernel relies on, the instance-major ray-bin tables (csrc/mrt_bin.h),
// and the byte total mrt_scene_info.device_bytes reports.  Built against host_build.cpp, host_texture.cpp and host_image.cpp
// (tests/test_device_image.py).
//   device_image <models dir> <bytes cornell> <bytes instanced> <bytes motion>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "mrt_image.h"

using namespace mrt;

static int g_fail = 0;
static const char* g_scene = "";
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (g_fail++ < 20) {                           \
                fprintf(stderr, "%s: ", g_scene);          \
                fprintf(stderr, __VA_ARGS__);              \
                fprintf(stderr, " [%s]\n", #cond);         \
            }                                              \
        }                                                  \
    } while (0)

static void must(int rc, const std::string& err, const char* what) {
    if (rc < 0) { fprintf(stderr, "%s: %s failed (%d): %s\n", g_scene, what, rc, err.c_str()); exit(2); }
}

static void base_scene(Scene& s) {
    DevMaterial m{};
    m.type = MRT_LAMBERT;
    m.kd[0] = m.kd[1] = m.kd[2] = 0.8f;
    m.ior = 1.5f; m.gloss = 1.f; m.sample_env = 1; m.env = -1; m.env_exposure = 1.f;
    for (int k = 0; k < 6; k++) m.maps[k] = -1;
    s.materials.push_back(m);
    DevLight l{};
    l.type = MRT_POINT_LIGHT;
    l.pos[1] = 10.f; l.power = 100.f; l.cast_shadows = 1; l.dome = -1;
    s.lights.push_back(l);
}

static int add_obj(Scene& s, const std::string& path) {
    Mesh m;
    std::string err;
    must(load_obj(path.c_str(), nullptr, m, err), err, path.c_str());
    m.material = 0;
    return s.push_mesh(std::move(m));
}

static void check_image(const Scene& s, const DeviceImage& g, size_t want_bytes) {
    const size_t nn = g.DN.size(), nl = g.DL.size(), nw = s.nodes.size();
    CHECK(nn > 0 && nl > 0, "empty image");
    CHECK(g.n_leaves_all == nl && g.world.n_nodes == nw && g.n_world == (int)s.obj_mesh.size(), "counts");
    for (size_t i = 0; i < nn; i++) {
        const QNode& q = g.DN[i];
        CHECK(q.pad[0] == slot_kinds(q.child), "node %zu: pad[0] %x", i, q.pad[0]);
        for (int k = 0; k < 4; k++) {
            const int32_t c = q.child[k];
            if (c == kEmptySlot) continue;
            if (c >= 0) { CHECK((size_t)c < nn, "node %zu slot %d: inner child %d of %zu", i, k, c, nn); continue; }
            const uint32_t w = ~(uint32_t)c, packet = w >> 4;   // the inverse of leaf_child
            CHECK(packet < nl, "node %zu slot %d: packet %u of %zu", i, k, packet, nl);
            if (packet >= nl) continue;
            const DLeaf& L = g.DL[packet];
            int used = 0;
            bool proxy = false;
            for (int j = 0; j < 4; j++) {
                if (L.prim[j] != -1) used = j + 1;
                proxy |= L.prim[j] <= -2;
            }
            CHECK((int)(w & 3u) + 1 == (used < 1 ? 1 : used), "node %zu slot %d: count %u, %d lanes used", i, k, (w & 3u) + 1, used);
            CHECK(((w & 4u) != 0) == proxy, "node %zu slot %d: proxy bit %u", i, k, w & 4u);
            CHECK(leaf_child(packet, (int)(w & 3u) + 1, (w & 4u) != 0, (w & 8u) != 0) == c, "node %zu slot %d: round trip", i, k);
        }
    }
    // the LDS renumbering: a permutation, and nodes 0 .. kLdsNodes - 1 breadth-first from the root in slot order
    CHECK(g.lds_ok == (nw >= (size_t)kLdsNodes), "lds_ok %d with %zu world nodes", (int)g.lds_ok, nw);
    CHECK(g.node_perm.size() == (g.lds_ok ? nw : 0), "node_perm holds %zu of %zu", g.node_perm.size(), nw);
    if (!g.node_perm.empty()) {
        std::vector<char> seen(nw, 0);
        for (int32_t p : g.node_perm) {
            CHECK(p >= 0 && (size_t)p < nw && !seen[(size_t)p], "node_perm: %d twice or out of range", p);
            if (p >= 0 && (size_t)p < nw) seen[(size_t)p] = 1;
        }
        std::vector<int32_t> bfs{0};
        std::vector<char> met(nw, 0);
        met[0] = 1;
        for (size_t q = 0; q < bfs.size() && bfs.size() < (size_t)kLdsNodes; q++)
            for (int k = 0; k < 4 && bfs.size() < (size_t)kLdsNodes; k++) {
                const int32_t c = g.DN[(size_t)bfs[q]].child[k];
                if (c < 0 || (size_t)c >= nw || met[(size_t)c]) continue;
                met[(size_t)c] = 1;
                bfs.push_back(c);
            }
        CHECK(bfs.size() == (size_t)kLdsNodes, "breadth-first walk met %zu nodes", bfs.size());
        for (size_t k = 0; k < bfs.size(); k++) CHECK(bfs[k] == (int32_t)k, "breadth-first node %zu has number %d", k, bfs[k]);
    }
    // instances and their BLASes
    CHECK(g.DI.size() == s.instances.size() && g.blas.size() == s.blas.size(), "instance / BLAS counts");
    for (size_t i = 0; i < g.DI.size(); i++) {
        const ImageInfo::BlasRange& B = g.blas[(size_t)s.instances[i].blas];
        CHECK(g.DI[i].root == (int32_t)B.tree.node_base && (size_t)g.DI[i].root >= nw && (size_t)g.DI[i].root < nn,
              "instance %zu: root %d, its BLAS at %u", i, g.DI[i].root, B.tree.node_base);
        CHECK(g.DI[i].shade_base == B.tree.shade_base, "instance %zu: shade_base", i);
    }
    for (size_t i = 0; i < g.PS.size(); i++) {
        const PrimShade& p = g.PS[i];
        if (p.pad) continue;   // a ProxyObject's own slot
        for (int k = 0; k < 3; k++)
            CHECK(p.v[k] < g.V.size() && p.n[k] < g.N.size(), "PrimShade %zu corner %d: v %u of %zu, n %u of %zu", i, k, p.v[k],
                  g.V.size(), p.n[k], g.N.size());
    }
    // time-1 vertices: V outside the motion-blurred meshes
    CHECK(g.V2.size() == (g.has_mb ? g.V.size() : 0) && g.PF.size() == (g.has_mb ? s.obj_mesh.size() : 0), "V2 / PF sizes");
    if (g.has_mb)
        for (size_t m = 0; m < s.meshes.size(); m++) {
            if (!s.meshes[m].verts2.empty()) continue;
            for (size_t i = 0; i < s.meshes[m].verts.size(); i++)
                CHECK(memcmp(&g.V2[g.vbase[m] + i], &g.V[g.vbase[m] + i], sizeof(F4)) == 0, "mesh %zu vertex %zu: V2 != V", m, i);
        }
    CHECK(g.bytes == want_bytes, "device bytes %zu, recorded %zu", g.bytes, want_bytes);
}

// The box of BLAS b from its own leaf packets in the image: the corners A, A + e0, A + e1 of every
// triangle.  *tol: what a corner rebuilt from the stored edges may differ from the vertex the
// build boxed: e = fl(B - A) and fl(A + e) round once each, at most an ulp of the largest
// coordinate together; 4 ulps are allowed.
static void blas_box(const DeviceImage& g, size_t b, float lo[3], float hi[3], float* tol) {
    const RefitTree& T = g.blas[b].tree;
    bool any = false;
    float big = 0.f;
    for (uint32_t p = T.leaf_base; p < T.leaf_base + T.n_leaves; p++)
        for (int j = 0; j < 4; j++) {
            const DLeaf& L = g.DL[p];
            if (L.prim[j] < 0) continue;
            for (int c = 0; c < 3; c++)
                for (int a = 0; a < 3; a++) {
                    const float x = c ? L.tri[j][a] + L.tri[j][3 * c + a] : L.tri[j][a];
                    lo[a] = any ? std::min(lo[a], x) : x;
                    hi[a] = any ? std::max(hi[a], x) : x;
                    big = std::max(big, fabsf(x));
                }
            any = true;
        }
    *tol = 4.f * 1.1920929e-7f * big;
}

// The instance-major ray-bin tables (csrc/mrt_bin.h): hit bases, classes, object-space cells
static void check_bin_tables(const Scene& s, const DeviceImage& g) {
    const size_t ni = g.DI.size();
    CHECK(g.hit_base.size() == ni && g.cls.size() == ni && g.cell.size() == 2 * ni, "table sizes %zu %zu %zu of %zu instances",
          g.hit_base.size(), g.cls.size(), g.cell.size(), ni);
    if (g.hit_base.size() != ni || g.cls.size() != ni || g.cell.size() != 2 * ni) return;
    for (size_t i = 0; i < ni; i++) {
        CHECK(g.hit_base[i] == g.DI[i].hit_base && g.hit_base[i] == s.instances[i].hit_base, "instance %zu: hit_base %d", i, g.hit_base[i]);
        CHECK(g.hit_base[i] >= g.n_world && (i == 0 || g.hit_base[i] > g.hit_base[i - 1]), "instance %zu: hit_base %d not ascending", i,
              g.hit_base[i]);
        // its class: its rank by BLAS root, then index, scaled to 0..127
        size_t rank = 0;
        for (size_t j = 0; j < ni; j++) rank += g.DI[j].root < g.DI[i].root || (g.DI[j].root == g.DI[i].root && j < i);
        CHECK(g.cls[i] == std::min<size_t>(127, rank * 128 / ni), "instance %zu: class %u at rank %zu of %zu", i, g.cls[i], rank, ni);
        // its cell: the low corner of its own BLAS's box + the BLAS bit, 4 / extent
        const size_t b = (size_t)s.instances[i].blas;
        float lo[3], hi[3], tol;
        blas_box(g, b, lo, hi, &tol);
        const F4 c0 = g.cell[2 * i], c1 = g.cell[2 * i + 1];
        const float got_lo[3] = {c0.x, c0.y, c0.z}, got_sc[3] = {c1.x, c1.y, c1.z};
        for (int a = 0; a < 3; a++) {
            const float ext = hi[a] - lo[a], want = 4.f / ext;
            CHECK(ext > 100.f * tol, "BLAS %zu axis %d: extent %g", b, a, ext);
            CHECK(fabsf(got_lo[a] - lo[a]) <= tol, "instance %zu axis %d: cell lo %.9g, BLAS %zu box lo %.9g (tol %g)", i, a, got_lo[a], b, lo[a], tol);
            CHECK(fabsf(got_sc[a] - want) <= want * (2.f * tol / ext + 4.f * 1.1920929e-7f), "instance %zu axis %d: cell scale %.9g, 4 / extent %.9g", i,
                  a, got_sc[a], want);
        }
        CHECK(c0.w == (float)(b & 1) && c1.w == 0.f, "instance %zu: BLAS bit %g of BLAS %zu, pad %g", i, c0.w, b, c1.w);
    }
}

// the boxes of two BLASes lie further apart than the tolerance of the cell check, so a cell
// taken from the wrong BLAS shows
static void check_blases_differ(const DeviceImage& g) {
    for (size_t b = 1; b < g.blas.size(); b++) {
        float lo0[3], hi0[3], lo1[3], hi1[3], t0, t1;
        blas_box(g, 0, lo0, hi0, &t0);
        blas_box(g, b, lo1, hi1, &t1);
        float far = 0.f;
        for (int a = 0; a < 3; a++) far = std::max(far, std::max(fabsf(lo0[a] - lo1[a]), fabsf((hi0[a] - lo0[a]) - (hi1[a] - lo1[a]))));
        CHECK(far > 1000.f * std::max(t0, t1), "BLAS 0 and %zu have the same box", b);
    }
}

static void run(const char* name, Scene& s, size_t want_bytes) {
    g_scene = name;
    std::string err;
    must(build_qbvh(s, err), err, "build_qbvh");
    DeviceImage g;
    must(build_image(s, g, err), err, "build_image");
    check_image(s, g, want_bytes);
    check_bin_tables(s, g);
    check_blases_differ(g);
    printf("%s: %zu nodes (%zu world), %zu packets, %zu instances, lds_ok %d, has_mb %d, %zu bytes\n", name, g.DN.size(),
           s.nodes.size(), g.DL.size(), g.DI.size(), (int)g.lds_ok, (int)g.has_mb, g.bytes);
}

int main(int argc, char** argv) {
    if (argc != 5) { fprintf(stderr, "usage: device_image <models dir> <bytes> <bytes> <bytes>\n"); return 2; }
    const std::string dir = std::string(argv[1]) + "/";
    std::string err;
    {   // fewer than kLdsNodes world nodes: no renumbering
        Scene s;
        base_scene(s);
        add_obj(s, dir + "cornell_box.obj");
        run("cornell", s, strtoull(argv[2], nullptr, 10));
    }
    {   // a world teapot, a BLAS of a second one with two instances and, between them, one instance of
        // a BLAS of the box (so the ray-bin tables can mix BLASes up): the renumbering is on
        Scene s;
        base_scene(s);
        add_obj(s, dir + "teapot.obj");
        const int32_t m = add_obj(s, dir + "teapot.obj");
        const int32_t b = make_blas(s, &m, 1, err);
        must(b, err, "make_blas");
        const int32_t m2 = add_obj(s, dir + "cornell_box.obj");
        const int32_t b2 = make_blas(s, &m2, 1, err);
        must(b2, err, "make_blas");
        for (int i = 0; i < 2; i++) {
            const float m16[16] = {1, 0, 0, 4.f * (float)(i + 1), 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
            must(add_instance(s, b, m16, err), err, "add_instance");
            const float box16[16] = {0, 0.5f, 0, -6, -0.5f, 0, 0, 1, 0, 0, 0.25f, 2, 0, 0, 0, 1};   // a quarter turn, scaled
            if (i == 0) must(add_instance(s, b2, box16, err), err, "add_instance");
        }
        run("instanced", s, strtoull(argv[3], nullptr, 10));
    }
    {   // a motion-blurred teapot (time-1 vertices 0.25 along x) beside a static box
        Scene s;
        base_scene(s);
        add_obj(s, dir + "cornell_box.obj");
        const int32_t m = add_obj(s, dir + "teapot.obj");
        Mesh& M = s.meshes[(size_t)m];
        M.verts2 = M.verts;
        for (v3& p : M.verts2) p.x += 0.25f;
        run("motion", s, strtoull(argv[4], nullptr, 10));
    }
    if (g_fail) fprintf(stderr, "%d checks failed\n", g_fail);
    return g_fail ? 1 : 0;
}
