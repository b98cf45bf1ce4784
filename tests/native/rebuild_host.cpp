// rebuild_host (csrc/host_build.cpp: mrt_scene_rebuild_bvh on the host) on the fixtures of
// tests/test_rebuild.py and three of tests/test_rebuild_shapes.py (a line at P = 513, a cloud at
// P = 1025, the key cell edges), without a GPU and without Python: built against host_build.cpp,
// host_texture.cpp and host_image.cpp with -fsanitize=address,undefined
// (tests/test_rebuild_native.py), so an index out of range or a read of freed memory ends the
// program.  After every rebuild (two per scene) the tree's own invariants are checked: every
// world prim once, compact packets, children numbered after their parent, every packet and
// node referenced once, at least two used slots per node, the enclosure, and a refit that
// changes nothing.
//   rebuild_host <models dir>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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
    for (int i = 0; i < 2; i++) {   // material 1 has an alpha map
        DevMaterial m{};
        m.type = MRT_LAMBERT;
        m.kd[0] = m.kd[1] = m.kd[2] = 0.8f;
        m.ior = 1.5f; m.gloss = 1.f; m.sample_env = 1; m.env = -1; m.env_exposure = 1.f;
        for (int k = 0; k < 6; k++) m.maps[k] = -1;
        s.materials.push_back(m);
    }
    Texture t;
    t.W = t.H = 2;
    t.type = kTexGray;
    t.rgb = {0.f, 1.f, 1.f, 0.f};
    s.textures.push_back(t);
    s.materials[1].maps[kMapAlpha] = 0;
    DevLight l{};
    l.type = MRT_POINT_LIGHT;
    l.pos[1] = 10.f; l.power = 100.f; l.cast_shadows = 1; l.dome = -1;
    s.lights.push_back(l);
}

// separate triangles: 9 floats each
static int add_soup(Scene& s, const std::vector<float>& tris, int material = 0) {
    Mesh m;
    m.material = material;
    for (size_t i = 0; i + 2 < tris.size(); i += 3) m.verts.push_back(mk(tris[i], tris[i + 1], tris[i + 2]));
    m.normals.push_back(mk(0.f, 0.f, 1.f));
    for (uint32_t i = 0; i < (uint32_t)m.verts.size(); i++) {
        m.vidx.push_back(i);
        m.nidx.push_back(0u);
    }
    return s.push_mesh(std::move(m));
}

static int add_obj(Scene& s, const std::string& path) {
    Mesh m;
    std::string err;
    must(load_obj(path.c_str(), nullptr, m, err), err, path.c_str());
    m.material = 0;
    return s.push_mesh(std::move(m));
}

static bool inside(const float* lo, const float* hi, const float* blo, const float* bhi) {
    for (int a = 0; a < 3; a++)
        if (!(blo[a] <= lo[a] && hi[a] <= bhi[a])) return false;
    return true;
}

static void check_tree(const Scene& s) {
    const size_t n = s.obj_mesh.size(), P = (n + 3) / 4, M = s.nodes.size();
    CHECK(s.leaves.size() == P, "%zu packets for %zu prims", s.leaves.size(), n);
    CHECK(M >= 1 && (P == 1 ? M == 1 : M <= P - 1), "%zu nodes for %zu packets", M, P);
    CHECK((size_t)s.info.nodes == M && (size_t)s.info.leaves == P && s.dev_dirty, "info");
    std::vector<int> seen(n, 0);
    for (size_t p = 0; p < s.leaves.size(); p++)
        for (int k = 0; k < 4; k++) {
            const int32_t o = s.leaves[p].prim[k];
            CHECK(o >= -1 && o < (int32_t)n, "packet %zu lane %d: prim %d", p, k, o);
            CHECK((o >= 0) == (4 * p + (size_t)k < n), "packet %zu lane %d: not compact", p, k);
            if (o >= 0 && o < (int32_t)n) seen[(size_t)o]++;
        }
    for (size_t o = 0; o < n; o++) CHECK(seen[o] == 1, "prim %zu in %d lanes", o, seen[o]);
    std::vector<int> node_refs(M, 0), leaf_refs(P, 0);
    for (size_t i = 0; i < M; i++) {
        const QNode& q = s.nodes[i];
        int used = 0;
        for (int k = 0; k < 4; k++) {
            const int32_t c = q.child[k];
            if (c == kEmptySlot) continue;
            CHECK(used == k, "node %zu: an empty slot before slot %d", i, k);
            used++;
            const float lo[3] = {q.box[k], q.box[4 + k], q.box[8 + k]}, hi[3] = {q.box[12 + k], q.box[16 + k], q.box[20 + k]};
            if (c >= 0) {
                CHECK((size_t)c > i && (size_t)c < M, "node %zu slot %d: child %d", i, k, c);
                if ((size_t)c >= M) continue;
                node_refs[(size_t)c]++;
                const QNode& ch = s.nodes[(size_t)c];
                for (int j = 0; j < 4; j++) {
                    if (ch.child[j] == kEmptySlot) continue;
                    const float clo[3] = {ch.box[j], ch.box[4 + j], ch.box[8 + j]}, chi[3] = {ch.box[12 + j], ch.box[16 + j], ch.box[20 + j]};
                    CHECK(inside(clo, chi, lo, hi), "node %zu slot %d does not hold its child's slot %d", i, k, j);
                }
            } else {
                CHECK((size_t)~c < P, "node %zu slot %d: packet %d", i, k, ~c);
                if ((size_t)~c >= P) continue;
                leaf_refs[(size_t)~c]++;
                for (int j = 0; j < 4; j++) {
                    const int32_t o = s.leaves[(size_t)~c].prim[j];
                    float fb[6];
                    if (o < 0) continue;
                    if (!fixed_lane_box(s, o, fb)) {
                        const Mesh& m = s.meshes[(size_t)s.obj_mesh[(size_t)o]];
                        for (int a = 0; a < 3; a++) fb[a] = 1e30f, fb[3 + a] = -1e30f;
                        for (int v = 0; v < 3; v++) {
                            const v3 p = m.verts[m.vidx[3 * (size_t)s.obj_tri[(size_t)o] + (size_t)v]];
                            const float x[3] = {p.x, p.y, p.z};
                            for (int a = 0; a < 3; a++) fb[a] = fminf(fb[a], x[a]), fb[3 + a] = fmaxf(fb[3 + a], x[a]);
                        }
                    }
                    CHECK(inside(fb, fb + 3, lo, hi), "node %zu slot %d does not hold prim %d", i, k, o);
                }
            }
        }
        CHECK(used >= (M == 1 && P == 1 ? 1 : 2), "node %zu has %d used slots", i, used);
    }
    for (size_t i = 1; i < M; i++) CHECK(node_refs[i] == 1, "node %zu has %d parents", i, node_refs[i]);
    for (size_t p = 0; p < P; p++) CHECK(leaf_refs[p] == 1, "packet %zu is in %d slots", p, leaf_refs[p]);
    // a refit at the same vertices changes no box and no triangle
    Scene& w = const_cast<Scene&>(s);
    const std::vector<QNode> N = s.nodes;
    const std::vector<QLeaf> L = s.leaves;
    refit_host(w);
    for (size_t i = 0; i < M; i++)
        for (int k = 0; k < 24; k++) CHECK(N[i].box[k] == s.nodes[i].box[k], "node %zu box %d moves under a refit", i, k);
    for (size_t p = 0; p < P; p++)
        for (int k = 0; k < 36; k++) CHECK(L[p].t[k] == s.leaves[p].t[k], "packet %zu value %d moves under a refit", p, k);
}

static void run(const char* name, Scene& s, size_t more_nodes_than_built = 0) {
    g_scene = name;
    std::string err;
    must(build_qbvh(s, err), err, "build_qbvh");
    const size_t built = s.nodes.size();
    const double c0 = bvh_cost_host(s);
    rebuild_host(s);
    check_tree(s);
    const size_t M = s.nodes.size();
    const double c1 = bvh_cost_host(s);
    if (more_nodes_than_built) CHECK(M > built && M == more_nodes_than_built, "%zu nodes, the built tree had %zu", M, built);
    rebuild_host(s);   // from the rebuilt state
    check_tree(s);
    DeviceImage g;   // and the image a re-upload would make of it
    must(build_image(s, g, err), err, "build_image");
    CHECK(g.world.n_nodes == s.nodes.size() && g.world.n_leaves == s.leaves.size(), "image counts");
    printf("%s: %zu prims, built %zu nodes (cost %.3f), rebuilt %zu nodes (cost %.3f), %zu packets\n", name, s.obj_mesh.size(),
           built, c0, M, c1, s.leaves.size());
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: rebuild_host <models dir>\n"); return 2; }
    const std::string dir = std::string(argv[1]) + "/";
    std::string err;
    {
        Scene s;
        base_scene(s);
        add_soup(s, {0, 0, 0, 1, 0, 0, 0, 1, 0});
        run("one triangle", s);
    }
    {
        Scene s;
        base_scene(s);
        std::vector<float> t;
        uint32_t x = 12345u;
        for (int i = 0; i < 45; i++) {
            x = x * 1664525u + 1013904223u;
            t.push_back((float)(x >> 8) / 16777216.f * 4.f - 2.f);
        }
        add_soup(s, t);
        run("five triangles", s);
    }
    {
        Scene s;
        base_scene(s);
        add_obj(s, dir + "teapot.obj");
        run("teapot", s);
    }
    {   // equal codes: the order comes from the position bits
        Scene s;
        base_scene(s);
        std::vector<float> t;
        for (int i = 0; i < 70; i++)
            for (float v : {0.f, 0.f, 0.f, 1.f, 0.f, 0.5f, 0.f, 1.f, 0.25f}) t.push_back(v);
        add_soup(s, t);
        run("70 identical triangles", s);
    }
    {   // every node binary: 63 nodes over 64 packets
        Scene s;
        base_scene(s);
        std::vector<float> t;
        for (int i = 0; i < 256; i++) {
            const float x = (float)i * 0.0625f;
            for (float v : {x, 0.f, 0.f, x + 0.01f, 0.f, 0.f, x, 0.01f, 0.01f}) t.push_back(v);
        }
        add_soup(s, t);
        run("256 triangles on a line", s, 63);
    }
    {   // the same at P = 513: 512 binary nodes, two levels of the segment tree at and below node 256
        Scene s;
        base_scene(s);
        std::vector<float> t;
        for (int i = 0; i < 2052; i++) {
            const float x = (float)i * 0.0625f;
            for (float v : {x, 0.f, 0.f, x + 0.05f, 0.f, 0.f, x, 0.05f, 0.01f}) t.push_back(v);
        }
        add_soup(s, t);
        run("2052 triangles on a line", s, 512);
    }
    {   // P = 1025: small triangles in a cube, nodes of two, three and four children
        Scene s;
        base_scene(s);
        std::vector<float> t;
        uint32_t x = 4097u;
        auto next = [&x]() {
            x = x * 1664525u + 1013904223u;
            return (float)(x >> 8) / 16777216.f;
        };
        for (int i = 0; i < 4097; i++) {
            const float c[3] = {next() * 6.f - 3.f, next() * 6.f - 3.f, next() * 6.f - 3.f};
            for (int v = 0; v < 3; v++)
                for (int a = 0; a < 3; a++) t.push_back(c[a] + next() * 0.1f - 0.05f);
        }
        add_soup(s, t);
        run("cloud of 4097 triangles", s);
    }
    {   // key cell edges: a triangle that spans the root box, and point triangles on, and one and two
        // floats to either side of, the edges of cells 0 .. 3, 511 .. 513 and 1022 .. 1024 of each axis
        Scene s;
        base_scene(s);
        const float lo[3] = {-1.f, 10.f, -0.3f}, hi[3] = {2.f, 10.7f, 0.9f};
        std::vector<float> t = {lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], lo[0], hi[1], lo[2]};
        for (int a = 0; a < 3; a++)
            for (int k : {0, 1, 2, 3, 511, 512, 513, 1022, 1023, 1024}) {
                float v = (float)((double)lo[a] + ((double)hi[a] - (double)lo[a]) * k / 1024.0);
                v = nextafterf(nextafterf(v, -INFINITY), -INFINITY);
                for (int j = 0; j < 5; j++, v = nextafterf(v, INFINITY)) {
                    float p[3] = {(float)(((double)lo[0] + hi[0]) / 2), (float)(((double)lo[1] + hi[1]) / 2),
                                  (float)(((double)lo[2] + hi[2]) / 2)};
                    p[a] = fminf(fmaxf(v, lo[a]), hi[a]);
                    for (int c = 0; c < 3; c++) t.insert(t.end(), {p[0], p[1], p[2]});
                }
            }
        add_soup(s, t);
        run("cell edges", s);
    }
    {   // no extent in y
        Scene s;
        base_scene(s);
        std::vector<float> t;
        for (int j = 0; j < 5; j++)
            for (int i = 0; i < 6; i++) {
                const float x = 0.75f * (float)i - 2.f, z = 0.5f * (float)j;
                for (float v : {x, 1.5f, z, x + 0.75f, 1.5f, z, x + 0.75f, 1.5f, z + 0.5f}) t.push_back(v);
                for (float v : {x, 1.5f, z, x + 0.75f, 1.5f, z + 0.5f, x, 1.5f, z + 0.5f}) t.push_back(v);
            }
        add_soup(s, t);
        run("flat mesh", s);
    }
    {   // all four lane kinds: a plain mesh, an alpha-mapped one, a motion-blurred one, three instances
        Scene s;
        base_scene(s);
        add_obj(s, dir + "cornell_box.obj");
        add_soup(s, {-3, 0.5f, 3, -1, 0.5f, 3, -1, 2.5f, 3, -3, 0.5f, 3, -1, 2.5f, 3, -3, 2.5f, 3}, 1);
        const int32_t mb = add_obj(s, dir + "sphere2.obj");
        s.meshes[(size_t)mb].verts2 = s.meshes[(size_t)mb].verts;
        for (v3& p : s.meshes[(size_t)mb].verts2) p.x += 0.25f;
        const int32_t m = add_obj(s, dir + "teapot.obj");
        const int32_t b = make_blas(s, &m, 1, err);
        must(b, err, "make_blas");
        for (int i = 0; i < 3; i++) {
            const float m16[16] = {1, 0, 0, 4.f * (float)(i + 1), 0, 1, 0, 0, 0, 0, 1, (float)i, 0, 0, 0, 1};
            must(add_instance(s, b, m16, err), err, "add_instance");
        }
        run("four lane kinds", s);
    }
    if (g_fail) fprintf(stderr, "%d checks failed\n", g_fail);
    return g_fail ? 1 : 0;
}
