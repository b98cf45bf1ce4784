// ref_driver -- runs the reference renderer's own classes on scenes this repository describes.
//
// TEST INFRASTRUCTURE ONLY (tests/test_reference_cpu.py, oracle/ref/make_reference_fixtures.py).
// Linked against the reference's translation units as oracle/ref/Makefile compiles them and
// against libmrt_oracle.so, of which it uses one function: oro_rand, to replay the oracle's
// counter-based random draws through the reference's random-number pool.
//
//   ref_driver load   OBJ OUT                     TriangleMesh::load's arrays, preCalc's tangent frames
//   ref_driver bvh    SCENE OUT                   QBVH node / leaf counts (2 x int32)
//   ref_driver trace  SCENE RAYS N SHADOW OUT     Scene::trace per ray (8 x 4 bytes per ray, see below)
//   ref_driver render SCENE OUT                   adaptiveSampleScene per pixel, free-running RNG
//   ref_driver replay SCENE OUT                   one sample per pixel on the oracle's draws
//   ref_driver repeat SCENE K OUT                 K free-running renders, one RNG stream running on
//   ref_driver replaylog SCENE LOG OUT            adaptiveSampleScene per pixel on the oracle's logged draws
//   ref_driver gamma  OUT                         Image::linear_to_gamma (32769 bytes), linear_to_gammaF (32769 floats)
//   ref_driver map    IN N OUT                    Map() of N floats: a 1-row image, setPixel, getCharPixels
//   ref_driver version                           the digest of the sources this driver was built from
//   ref_driver decode FILE OUT                    RawImage::loadImage: width, height, channels (int32), the floats
//
// SCENE is the text format oracle/refdriver.py writes: one command per line, integers in
// decimal, floats as the 8 hex digits of their bits, arrays in raw little-endian side files.
// Single-threaded by construction: every call passes thread 0 (run with OMP_NUM_THREADS=1).
#include <stdint.h>
#include <fstream>
#include <limits>
#include <map>
#include <new>
#include <sstream>
#include <string>
#include <vector>

#include "Miro.h"
#include "Scene.h"
#include "Camera.h"
#include "Image.h"
#include "PointLight.h"
#include "RectangleLight.h"
#include "DomeLight.h"
#include "Object.h"
#include "ProxyObject.h"
#include "MBObject.h"
#include "TriangleMesh.h"
#include "Lambert.h"
#include "Blinn.h"
#include "RawImage.h"
#include "Texture.h"
#include "BVH.h"

#ifndef DRIVER_SUM
#define DRIVER_SUM "unknown"
#endif

extern "C" float oro_rand(uint32_t pixel, uint32_t sample, uint32_t dim, uint32_t seed);

namespace {

struct Tok {
    std::istringstream in;
    explicit Tok(const std::string& line) : in(line) {}
    std::string word() { std::string w; if (!(in >> w)) die("missing token"); return w; }
    int integer() { return atoi(word().c_str()); }
    float real() { uint32_t u = (uint32_t)strtoul(word().c_str(), 0, 16); float f; memcpy(&f, &u, 4); return f; }
    Vector3 vec() { float x = real(), y = real(), z = real(); return Vector3(x, y, z); }
    static void die(const char* what) { fprintf(stderr, "ref_driver: %s\n", what); exit(2); }
};

std::vector<char> slurp(const std::string& path, size_t want) {
    std::vector<char> buf(want);
    FILE* f = fopen(path.c_str(), "rb");
    if (!f || fread(buf.data(), 1, want, f) != want) { fprintf(stderr, "ref_driver: cannot read %zu bytes of %s\n", want, path.c_str()); exit(2); }
    fclose(f);
    return buf;
}

void spill(const std::string& path, const void* p, size_t n) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f || fwrite(p, 1, n, f) != n) { fprintf(stderr, "ref_driver: cannot write %s\n", path.c_str()); exit(2); }
    fclose(f);
}

TriangleMesh* new_mesh() {
    TriangleMesh* m = new TriangleMesh;
    m->m_tangents = 0; m->m_biTangents = 0;     // its constructor leaves these two unset
    return m;
}

struct MeshEntry { TriangleMesh* mesh; TriangleMesh* mesh2; Material* mat; bool in_blas; };
struct Blas { Objects* objs; BVH* bvh; std::map<const Object*, int> index; };
struct World { int mesh; int blas; Matrix4x4 m; };     // mesh >= 0: a mesh's triangles; else an instance

struct Loaded {
    Camera* cam;
    Image* img;
    int W, H;
    std::vector<Material*> mats;
    std::vector<MeshEntry> meshes;
    std::vector<Texture*> tex;
    std::vector<Blas> blas;
    std::vector<World> world;
    std::map<const Object*, int> index;          // world object -> position in Scene::objects()
    std::map<const Object*, int> proxy_blas;     // ProxyObject -> its BLAS
};

ImageType image_type(int oracle_type) {         // oracle: 0 HDR, 1 grey, 3 RGB, 4 RGBA
    switch (oracle_type) {
        case 0: return HDR;
        case 1: return GRAYSCALE;
        case 3: return RGB;
        case 4: return RGBA;
    }
    Tok::die("bad texture type");
    return RGB;
}

void load_scene(const char* path, Loaded& S) {
    g_scene = new Scene;
    g_image = S.img = new Image;
    g_camera = S.cam = new (_aligned_malloc(sizeof(Camera), 16)) Camera;
    S.W = S.H = 1;
    std::ifstream f(path);
    if (!f) Tok::die("cannot open scene file");
    std::string line;
    while (std::getline(f, line)) {
        if (line.empty() || line[0] == '#') continue;
        Tok t(line);
        const std::string cmd = t.word();
        if (cmd == "material") {
            const int blinn = t.integer();
            Vector3 kd = t.vec(), ka = t.vec(), ks = t.vec();
            float specExp = t.real(), specAmt = t.real(), reflect = t.real(), refract = t.real(), ior = t.real();
            float gloss = t.real(), translucency = t.real();
            Vector3 le = t.vec();
            float emitted = t.real();
            int sampleEnv = t.integer(), disperse = t.integer();
            float i0 = t.real(), i1 = t.real(), i2 = t.real();
            Material* m;
            if (!blinn) m = new Lambert(kd, ka);
            else {
                Blinn* b = new Blinn(kd, ka, ks, Vector3(0.f), ior, specExp, specAmt, reflect, refract, gloss, emitted, le);
                b->setRefractAmt(refract);
                b->setLightEmittedIntensity(emitted); b->setLightEmittedColor(le);   // its constructor zeroes both
                b->setIor(i0, 0); b->setIor(i1, 1); b->setIor(i2, 2);
                b->setTranslucency(translucency);
                b->setSampleEnv(sampleEnv != 0);
                b->m_disperse = disperse != 0;
                m = b;
            }
            S.mats.push_back(m);
        } else if (cmd == "mesh") {
            int nv = t.integer(), nn = t.integer(), nt = t.integer(), mat = t.integer();
            std::vector<char> raw = slurp(t.word(), (size_t)(nv + nn) * 12 + (size_t)nt * 24);
            const float* fp = (const float*)raw.data();
            TriangleMesh* m = new_mesh();
            m->m_vertices = new Vector3[nv ? nv : 1];
            m->m_normals = new Vector3[nn ? nn : 1];
            for (int i = 0; i < nv; i++, fp += 3) m->m_vertices[i] = Vector3(fp[0], fp[1], fp[2]);
            for (int i = 0; i < nn; i++, fp += 3) m->m_normals[i] = Vector3(fp[0], fp[1], fp[2]);
            const uint32_t* ip = (const uint32_t*)fp;
            m->m_vertexIndices = new TriangleMesh::TupleI3[nt ? nt : 1];
            m->m_normalIndices = new TriangleMesh::TupleI3[nt ? nt : 1];
            for (int i = 0; i < nt; i++, ip += 3) { m->m_vertexIndices[i].x = ip[0]; m->m_vertexIndices[i].y = ip[1]; m->m_vertexIndices[i].z = ip[2]; }
            for (int i = 0; i < nt; i++, ip += 3) { m->m_normalIndices[i].x = ip[0]; m->m_normalIndices[i].y = ip[1]; m->m_normalIndices[i].z = ip[2]; }
            m->m_numTris = nt;
            S.world.push_back(World{(int)S.meshes.size(), -1, Matrix4x4()});
            S.meshes.push_back(MeshEntry{m, 0, S.mats.at(mat), false});
        } else if (cmd == "obj") {
            int mat = t.integer();
            std::string p = t.word();
            TriangleMesh* m = new_mesh();
            if (!m->load((char*)p.c_str())) Tok::die("OBJ load failed");
            S.world.push_back(World{(int)S.meshes.size(), -1, Matrix4x4()});
            S.meshes.push_back(MeshEntry{m, 0, S.mats.at(mat), false});
        } else if (cmd == "texcoords") {
            int mesh = t.integer(), ntc = t.integer();
            TriangleMesh* m = S.meshes.at(mesh).mesh;
            std::vector<char> raw = slurp(t.word(), (size_t)ntc * 8 + (size_t)m->m_numTris * 12);
            const float* fp = (const float*)raw.data();
            m->m_texCoords = (TriangleMesh::VectorR2*)_aligned_malloc(sizeof(TriangleMesh::VectorR2) * (ntc ? ntc : 1), 16);
            for (int i = 0; i < ntc; i++, fp += 2) { m->m_texCoords[i].x = fp[0]; m->m_texCoords[i].y = fp[1]; }
            const uint32_t* ip = (const uint32_t*)fp;
            m->m_texCoordIndices = new TriangleMesh::TupleI3[m->m_numTris ? m->m_numTris : 1];
            for (u_int i = 0; i < m->m_numTris; i++, ip += 3) { m->m_texCoordIndices[i].x = ip[0]; m->m_texCoordIndices[i].y = ip[1]; m->m_texCoordIndices[i].z = ip[2]; }
        } else if (cmd == "motion") {
            int mesh = t.integer(), nv = t.integer();
            MeshEntry& e = S.meshes.at(mesh);
            std::vector<char> raw = slurp(t.word(), (size_t)nv * 12);
            const float* fp = (const float*)raw.data();
            TriangleMesh* m2 = new_mesh();       // time 1: same topology, other vertices
            *m2 = *e.mesh;
            m2->m_vertices = new Vector3[nv ? nv : 1];
            for (int i = 0; i < nv; i++, fp += 3) m2->m_vertices[i] = Vector3(fp[0], fp[1], fp[2]);
            e.mesh2 = m2;
        } else if (cmd == "texture") {
            int w = t.integer(), h = t.integer(), type = t.integer(), ch = t.integer();
            std::vector<char> raw = slurp(t.word(), (size_t)w * h * ch * 4);
            float* data = new float[(size_t)w * h * ch];
            memcpy(data, raw.data(), raw.size());
            S.tex.push_back(new Texture(new RawImage(w, h, data, image_type(type))));
        } else if (cmd == "maps") {
            Material* m = S.mats.at(t.integer());
            int id[6];
            for (int i = 0; i < 6; i++) id[i] = t.integer();
            if (id[0] >= 0) m->setColorMap(S.tex.at(id[0]));
            if (id[1] >= 0) m->setNormalMap(S.tex.at(id[1]));
            if (id[2] >= 0) m->setSpecularMap(S.tex.at(id[2]));
            if (id[3] >= 0) m->setReflectMap(S.tex.at(id[3]));
            if (id[4] >= 0) m->setRefractMap(S.tex.at(id[4]));
            if (id[5] >= 0) m->setAlphaMap(S.tex.at(id[5]));
        } else if (cmd == "light") {
            const std::string kind = t.word();
            Light* l;
            if (kind == "point") {
                PointLight* p = new PointLight;
                p->setPosition(t.vec()); p->setPower(t.real());
                l = p;
            } else if (kind == "rect") {
                RectangleLight* r = new RectangleLight;
                Vector3 a = t.vec(), b = t.vec(), c = t.vec();
                r->setVertices(a, b, c); r->setPower(t.real());
                l = r;
            } else {
                DomeLight* d = new DomeLight;
                d->setTexture(S.tex.at(t.integer())); d->setPower(t.real());
                l = d;
            }
            l->setSamples(t.integer()); l->setNoiseThreshold(t.real());
            l->setCastShadows(t.integer() != 0); l->setFastShadows(t.integer() != 0);
            g_scene->addLight(l);
        } else if (cmd == "blas") {                // ProxyObject::setupMultiProxy over whole meshes
            int n = t.integer();
            std::vector<TriangleMesh*> ms; std::vector<Material*> mt;
            for (int i = 0; i < n; i++) {
                int id = t.integer();
                S.meshes.at(id).in_blas = true;
                ms.push_back(S.meshes[id].mesh); mt.push_back(S.meshes[id].mat);
            }
            Blas b; b.objs = new Objects; b.bvh = new BVH;
            ProxyObject::setupMultiProxy(ms.data(), n, mt.data(), b.objs, b.bvh);
            for (size_t i = 0; i < b.objs->size(); i++) b.index[(*b.objs)[i]] = (int)i;
            S.blas.push_back(b);
        } else if (cmd == "instance") {
            int b = t.integer();
            Matrix4x4 m;
            float* rows[4] = {m.m1, m.m2, m.m3, m.m4};
            for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) rows[r][c] = t.real();
            S.world.push_back(World{-1, b, m});
        } else if (cmd == "bg") {
            Vector3 c = t.vec();
            g_scene->setBGColor(c);
        } else if (cmd == "envmap") {
            int id = t.integer();
            g_scene->setEnvMap(id >= 0 ? S.tex.at(id) : 0); g_scene->setEnvExposure(t.real());
        } else if (cmd == "matenv") {
            Material* m = S.mats.at(t.integer());
            int id = t.integer();
            m->setEnvMap(id >= 0 ? S.tex.at(id) : 0); m->setEnvExposure(t.real());
        } else if (cmd == "numpaths") {
            g_scene->setNumPaths(t.integer());
        } else if (cmd == "pathtrace") {
            g_scene->setPathTrace(t.integer() != 0); g_scene->setMaxBounces(t.integer()); g_scene->setSampleEnv(t.integer() != 0);
        } else if (cmd == "subdivs") {
            g_scene->setMinSubdivs(t.integer()); g_scene->setMaxSubdivs(t.integer()); g_scene->setNoise(t.real());
        } else if (cmd == "camera") {
            Vector3 eye = t.vec(), up = t.vec(), look = t.vec();
            S.cam->setEye(eye); S.cam->setLookAt(look); S.cam->setUp(up); S.cam->setFOV(t.real());
            S.cam->setAperture(t.real()); S.cam->setFocusPlane(t.real()); S.cam->setShutterSpeed(t.real());
        } else if (cmd == "size") {
            S.W = t.integer(); S.H = t.integer();
            S.img->resize(S.W, S.H);
        } else {
            Tok::die(("unknown scene command " + cmd).c_str());
        }
    }
    // the world's objects in add order: a mesh's triangles first to last (makeMeshObjs /
    // makeMBMeshObjs of the reference's scene scripts), one ProxyObject per instance
    for (size_t w = 0; w < S.world.size(); w++) {
        const World& e = S.world[w];
        if (e.mesh >= 0) {
            const MeshEntry& me = S.meshes[e.mesh];
            if (me.in_blas) continue;
            for (u_int i = 0; i < me.mesh->m_numTris; i++)
                g_scene->addObject(me.mesh2 ? new MBObject(me.mat, me.mesh, me.mesh2, i) : new Object(me.mat, me.mesh, i));
        } else {
            Blas& b = S.blas.at(e.blas);
            ProxyObject* p = new ProxyObject(b.objs, b.bvh, e.m);
            S.proxy_blas[p] = e.blas;
            g_scene->addObject(p);
        }
    }
    g_scene->preCalc();
    const Objects& os = *g_scene->objects();
    for (size_t i = 0; i < os.size(); i++) S.index[os[i]] = (int)i;
}

struct HitRecord { int32_t hit; float t, a, b; int32_t obj, proxy; uint32_t nodes, leaves; };

// Scene::trace for one ray.  obj: position of the hit object in the world's objects, or in
// its instance's objects when proxy (the instance's position in the world's objects) >= 0.
HitRecord trace_one(const Loaded& S, const float* r, bool shadow) {
    Ray ray(0, Vector3(r[0], r[1], r[2]), Vector3(r[3], r[4], r[5]), 0.f, 1.001f, 0, 0, shadow ? IS_SHADOW_RAY : IS_PRIMARY_RAY);
    HitInfo h(r[7]);
    const unsigned long b0 = BVH::rayBoxIntersections[0], t0 = Ray::rayTriangleIntersections[0];
    HitRecord out;
    out.hit = g_scene->trace(0, h, ray, r[6]) ? 1 : 0;
    out.nodes = (uint32_t)(BVH::rayBoxIntersections[0] - b0);
    out.leaves = (uint32_t)(Ray::rayTriangleIntersections[0] - t0);
    out.t = h.t; out.a = h.a; out.b = h.b; out.obj = -1; out.proxy = -1;
    if (out.hit && !shadow) {
        if (h.m_proxy) {
            out.proxy = S.index.at(h.m_proxy);
            out.obj = S.blas[S.proxy_blas.at(h.m_proxy)].index.at(h.obj);
        } else {
            out.obj = S.index.at(h.obj);
        }
    }
    return out;
}

// one frame in the reference's own pixel order (buckets row-major, rows, then columns)
template <class PerPixel> void for_each_pixel(int W, int H, PerPixel fn) {
    const int nx = W / bucket_size + (W % bucket_size > 0), ny = H / bucket_size + (H % bucket_size > 0);
    for (int bucket = 0; bucket < nx * ny; bucket++) {
        const int bx = bucket % nx, by = bucket / nx;
        for (int j = by * bucket_size; j < std::min((by + 1) * bucket_size, H); ++j)
            for (int i = bx * bucket_size; i < std::min((bx + 1) * bucket_size, W); ++i) fn(i, j);
    }
}

void render_frame(Loaded& S, float* rgb) {
    Ray ray(0);
    HitInfo hit;
    for_each_pixel(S.W, S.H, [&](int i, int j) {
        Vector3 c = g_scene->adaptiveSampleScene(0, S.cam, S.img, ray, hit, i, j);
        float* p = rgb + 3 * ((size_t)j * S.W + i);
        p[0] = c.x; p[1] = c.y; p[2] = c.z;
    });
}

// One sample per pixel on the oracle's draws: the camera's draws are the oracle's dims
// 0.. of (pixel, sample 0), the shade() call's are dims (1 << 24) + k; the pool's read
// position after eyeRayAdaptive says how many the camera took (depth of field varies).
void replay_frame(Loaded& S, float* rgb) {
    const uint32_t seed = 0x5EEDu;
    const int CAMERA_DRAWS = 256, SHADE_DRAWS = 8192;
    Ray ray(0);
    HitInfo hit;
    for_each_pixel(S.W, S.H, [&](int i, int j) {
        const uint32_t pixel = (uint32_t)(j * S.W + i);
        for (int k = 0; k < CAMERA_DRAWS; k++) Scene::rands[k] = oro_rand(pixel, 0, (uint32_t)k, seed);
        Scene::randsIdx[0] = 0;
        ray = S.cam->eyeRayAdaptive(0, i, j, 0.5f, 0.5f, 0.5f, 0.5f, S.W, S.H);
        const int used = Scene::randsIdx[0];
        if (used > CAMERA_DRAWS) Tok::die("camera drew past the replayed draws");
        for (int k = 0; k < SHADE_DRAWS; k++) Scene::rands[used + k] = oro_rand(pixel, 0, (1u << 24) + (uint32_t)k, seed);
        Vector3 c = g_scene->sampleScene(0, ray, hit);
        if (Scene::randsIdx[0] > used + SHADE_DRAWS || Scene::randsIdx[0] < used) Tok::die("shading drew past the replayed draws");
        float* p = rgb + 3 * ((size_t)j * S.W + i);
        p[0] = c.x; p[1] = c.y; p[2] = c.z;
    });
}

// Every chain level on the oracle's draws.  LOG: W*H uint32 draw counts (pixels row-major), then
// (skey, dim) uint32 pairs of every draw in the oracle's call order.  The oracle's next_rand sites
// are in the order of the reference's getRand sites, so pixel p's k-th logged key is the k-th value
// the reference reads from the pool: the pool gets oro_rand of those keys, NaN after them (a draw
// too many shows in the colour), and the whole of adaptiveSampleScene runs from read position 0.
// OUT: W*H*3 floats, the W*H*3 bytes Image::setPixel stored, W*H uint32 draws consumed.
void replay_log_frame(Loaded& S, const char* log_path, const char* out_path) {
    const uint32_t seed = 0x5EEDu;
    const int POOL = 65536;                        // thread 0's pool; getRand regenerates it at this read position
    const size_t np = (size_t)S.W * S.H;
    std::vector<char> head = slurp(log_path, np * 4);
    const uint32_t* counts = (const uint32_t*)head.data();
    std::vector<uint64_t> first(np + 1, 0);
    for (size_t p = 0; p < np; p++) {
        if (counts[p] >= (uint32_t)POOL) Tok::die("a pixel logs 65536 draws or more: the pool wraps there");
        first[p + 1] = first[p] + counts[p];
    }
    std::vector<char> raw = slurp(log_path, np * 4 + first[np] * 8);
    const uint32_t* keys = (const uint32_t*)(raw.data() + np * 4);
    std::vector<float> rgb(np * 3);
    std::vector<uint32_t> consumed(np);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    Ray ray(0);
    HitInfo hit;
    for_each_pixel(S.W, S.H, [&](int i, int j) {
        const size_t p = (size_t)j * S.W + i;
        const uint32_t* k = keys + 2 * first[p];
        const int n = (int)counts[p];
        for (int d = 0; d < n; d++) Scene::rands[d] = oro_rand((uint32_t)p, k[2 * d], k[2 * d + 1], seed);
        for (int d = n; d < POOL; d++) Scene::rands[d] = nan;
        Scene::randsIdx[0] = 0;
        Vector3 c = g_scene->adaptiveSampleScene(0, S.cam, S.img, ray, hit, i, j);
        consumed[p] = (uint32_t)Scene::randsIdx[0];
        S.img->setPixel(i, j, c);
        rgb[3 * p] = c.x; rgb[3 * p + 1] = c.y; rgb[3 * p + 2] = c.z;
    });
    std::vector<char> out((const char*)rgb.data(), (const char*)(rgb.data() + rgb.size()));
    const char* px = (const char*)S.img->getCharPixels();
    out.insert(out.end(), px, px + np * 3);
    out.insert(out.end(), (const char*)consumed.data(), (const char*)(consumed.data() + np));
    spill(out_path, out.data(), out.size());
}

int cmd_gamma(const char* out_path) {
    Image img;                                     // its constructor runs generateGammaTables
    std::vector<char> out((const char*)Image::linear_to_gamma, (const char*)Image::linear_to_gamma + 32769);
    out.insert(out.end(), (const char*)Image::linear_to_gammaF, (const char*)(Image::linear_to_gammaF + 32769));
    spill(out_path, out.data(), out.size());
    return 0;
}

int cmd_map(const char* in_path, int n, const char* out_path) {
    std::vector<char> raw = slurp(in_path, (size_t)n * 4);
    const float* x = (const float*)raw.data();
    Image img;
    img.resize(n, 1);
    for (int i = 0; i < n; i++) img.setPixel(i, 0, Vector3(x[i], x[i], x[i]));
    spill(out_path, img.getCharPixels(), (size_t)n * 3);
    return 0;
}

// RawImage::loadImage, the loader behind every Texture of the reference's scene scripts (material
// maps and Scene::setEnvMap alike); TGA decoding reads Image::gamma_to_linear, so an Image first.
int cmd_decode(char* file, const char* out_path) {
    Image img;
    RawImage r;
    r.m_rawData = 0; r.m_width = r.m_height = 0;
    r.loadImage(file);
    if (!r.m_rawData || r.m_width <= 0 || r.m_height <= 0) return 3;
    const int32_t ch = r.m_imageType == GRAYSCALE ? 1 : r.m_imageType == RGBA ? 4 : 3;
    const int32_t head[3] = {r.m_width, r.m_height, ch};
    std::vector<char> out((const char*)head, (const char*)(head + 3));
    out.insert(out.end(), (const char*)r.m_rawData, (const char*)(r.m_rawData + (size_t)r.m_width * r.m_height * ch));
    spill(out_path, out.data(), out.size());
    return 0;
}

// TriangleMesh::load and TriangleMesh::preCalc of one OBJ.  The mesh keeps no array lengths, so
// they are recounted here from the file the way the loader sizes its arrays (lines that begin
// "v", "vn", "vt"); a file without normals gets the loader's own, counted by the indices.
int cmd_load(char** a) {
    TriangleMesh* m = new_mesh();
    if (!m->load(a[0])) return 3;
    const u_int nt = m->m_numTris;
    uint32_t nv = 0, nn = 0, ntc = 0;
    std::ifstream f(a[0]);
    for (std::string line; std::getline(f, line);) {
        if (line.size() < 2 || line[0] != 'v') continue;
        if (line[1] == 'n') nn++; else if (line[1] == 't') ntc++; else nv++;
    }
    if (!nn) for (u_int i = 0; i < nt; i++) {
        const TriangleMesh::TupleI3& t = m->m_normalIndices[i];
        nn = std::max(nn, std::max(t.x, std::max(t.y, t.z)) + 1);
    }
    const bool has_tc = m->m_texCoordIndices != 0;
    m->preCalc();                      // with texture coordinates: the tangent frames, per normal slot
    const bool has_tan = has_tc && m->m_tangents && nn <= 3 * nt;
    std::vector<uint32_t> head = {nt, (uint32_t)has_tc, nv, nn, ntc, (uint32_t)has_tan};
    std::vector<char> out((const char*)head.data(), (const char*)(head.data() + head.size()));
    auto put = [&](const void* p, size_t n) { out.insert(out.end(), (const char*)p, (const char*)p + n); };
    for (u_int i = 0; i < nv; i++) put(&m->m_vertices[i].x, 12);
    for (u_int i = 0; i < nn; i++) put(&m->m_normals[i].x, 12);
    for (u_int i = 0; i < nt; i++) put(&m->m_vertexIndices[i], 12);
    for (u_int i = 0; i < nt; i++) put(&m->m_normalIndices[i], 12);
    if (has_tc) {
        for (u_int i = 0; i < ntc; i++) put(&m->m_texCoords[i], 8);
        for (u_int i = 0; i < nt; i++) put(&m->m_texCoordIndices[i], 12);
    }
    if (has_tan) {
        for (u_int i = 0; i < nn; i++) put(&m->m_tangents[i].x, 12);
        for (u_int i = 0; i < nn; i++) put(&m->m_biTangents[i].x, 12);
    }
    spill(a[1], out.data(), out.size());
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && std::string(argv[1]) == "version") { puts(DRIVER_SUM); return 0; }
    if (argc < 3) Tok::die("usage: ref_driver COMMAND ...");
    const std::string cmd = argv[1];
    if (cmd == "load" && argc == 4) return cmd_load(argv + 2);
    if (cmd == "gamma" && argc == 3) return cmd_gamma(argv[2]);
    if (cmd == "map" && argc == 5) return cmd_map(argv[2], atoi(argv[3]), argv[4]);
    if (cmd == "decode" && argc == 4) return cmd_decode(argv[2], argv[3]);
    Loaded S;
    load_scene(argv[2], S);
    if (cmd == "bvh" && argc == 4) {
        int32_t n[2] = {(int32_t)QBVH_Node::nodeCount, (int32_t)QBVH_Node::leafCount};
        spill(argv[3], n, sizeof n);
    } else if (cmd == "trace" && argc == 7) {
        const size_t n = (size_t)atol(argv[4]);
        const bool shadow = atoi(argv[5]) != 0;
        std::vector<char> raw = slurp(argv[3], n * 32);
        std::vector<HitRecord> out(n);
        for (size_t i = 0; i < n; i++) out[i] = trace_one(S, (const float*)raw.data() + 8 * i, shadow);
        spill(argv[6], out.data(), n * sizeof(HitRecord));
    } else if ((cmd == "render" || cmd == "replay") && argc == 4) {
        std::vector<float> rgb((size_t)S.W * S.H * 3);
        if (cmd == "render") render_frame(S, rgb.data()); else replay_frame(S, rgb.data());
        spill(argv[3], rgb.data(), rgb.size() * 4);
    } else if (cmd == "replaylog" && argc == 5) {
        replay_log_frame(S, argv[3], argv[4]);
    } else if (cmd == "repeat" && argc == 5) {
        const int K = atoi(argv[3]);
        std::vector<float> rgb((size_t)K * S.W * S.H * 3);
        for (int k = 0; k < K; k++) render_frame(S, rgb.data() + (size_t)k * S.W * S.H * 3);
        spill(argv[4], rgb.data(), rgb.size() * 4);
    } else {
        Tok::die("bad command line");
    }
    return 0;
}
