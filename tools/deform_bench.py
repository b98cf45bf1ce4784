"""Deform against rebuild: what does mrt_scene_deform_mesh cost for a mesh of a BLAS next to the
only route there was before it, a new scene with the new vertices + the BLAS builds +
mrt_scene_build_bvh + mrt_scene_upload?  (One process, one device; needs the GPU.)

    python tools/deform_bench.py [C5 FS ...] [--rounds R] [--frame-rounds Q] [--frame-reps K] [--out FILE]

Scenes: C5, whose buddha stand-in BLAS (the BLAS with the most triangles) is deformed, and FS
(the reference's final scene), whose grass-blade BLAS (the BLAS with the most instances) is.
Every vertex of the BLAS's first mesh moves by a seeded displacement of up to 1% of the mesh's
largest extent, the deforms alternating between two such sets; the normals stay.  Per scene,
after a clock-settle period of untimed frames, medians over R rounds of
  refit_ms           device events around the kernels of the synchronous entry (scatter, the
                     BLAS's leaf kernel and node kernels, the instance box kernel, the world's
                     leaf kernel and node kernels)
  refit_wall_ms      wall time of the synchronous mrt_scene_deform_mesh
  refit_async_ms     device events around mrt_scene_deform_mesh_async on a device tensor (null
                     for a mesh with texture coordinates, which the async form refuses)
  rebuild_upload_ms  the route it replaces, in the same run: a second scene object given the new
                     vertices, everything added again (the BLAS builds included), then
                     mrt_scene_build_bvh and mrt_scene_upload; world_build_ms / blas_build_ms
                     are the two builds inside it
  frame_refit_ms / frame_fresh_ms   device time of a frame (mrt_render_frame_async, K back to
                     back) on the refitted trees and on the fresh build at the same vertices,
                     alternating (Q rounds)
the share of pixels whose hit (prim, t) agrees between the two, and the launch count of one
deform.  A frame is rendered between the timed deforms where a frame takes under 0.1 s.  Writes
a JSON list (default profiles/deform_bench.json) and prints one line per scene."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rendering-algorithms-raytracer_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import miro  # noqa: E402
from miro import _lib, scenes  # noqa: E402

SETTLE_S = 0.5
FRAME_REPS = 3


def opt(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def note(msg):
    print("[deform_bench] " + msg, file=sys.stderr, flush=True)


def med(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def mesh_table(scene):
    """Scene.preCalc's numbering restated: (mesh objects by mesh id, mesh ids by BLAS id)."""
    meshes, blas, seen = [], [], {}
    for entry in scene._meshes:
        item = entry[0]
        if not isinstance(item, miro.ProxyObject):
            meshes.append(item)
            continue
        if id(item.bvh) not in seen:
            seen[id(item.bvh)] = len(blas)
            blas.append(list(range(len(meshes), len(meshes) + len(item.bvh.objects))))
            meshes.extend(m for m, _ in item.bvh.objects)
    return meshes, blas


def blas_counts(scene, n_blas):
    L = miro.lib()
    out = []
    for b in range(n_blas):
        n, lv, p = C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(L.mrt_scene_blas_info(scene.handle, b, C.byref(n), C.byref(lv), C.byref(p)), "blas_info")
        out.append(dict(nodes=n.value, leaves=lv.value, prims=p.value))
    return out


def heights(node_child):
    h = np.zeros(len(node_child), np.int64)
    for i in range(len(node_child) - 1, -1, -1):
        c = node_child[i][node_child[i] >= 0]
        if len(c):
            h[i] = h[c].max() + 1
    return int(h.max()) + 1


def texcoords(scene, mesh_id):
    L = miro.lib()
    n = C.c_int32()
    _lib.check(L.mrt_scene_mesh_texcoords(scene.handle, mesh_id, C.byref(n), None, None), "texcoords")
    if not n.value:
        return None
    nt = len(scene.mesh_arrays(mesh_id)[2])
    uv, tidx = np.zeros((n.value, 2), np.float32), np.zeros((nt, 3), np.uint32)
    _lib.check(L.mrt_scene_mesh_texcoords(scene.handle, mesh_id, C.byref(n), uv.ctypes.data_as(C.POINTER(C.c_float)),
                                          tidx.ctypes.data_as(C.POINTER(C.c_uint32))), "texcoords")
    return uv, tidx


def moved(V, seed):
    """V + a seeded displacement per vertex, uniform in a ball of 1% of the largest extent."""
    rng = np.random.default_rng(seed)
    ext = float((V.max(0) - V.min(0)).max())
    u = rng.normal(size=V.shape)
    u *= (rng.uniform(0, 1, (len(V), 1)) ** (1 / 3)) / np.linalg.norm(u, axis=1, keepdims=True)
    return np.ascontiguousarray(V + 0.01 * ext * u, np.float32)


def measure(key, rounds, frame_rounds, frame_reps):
    L = miro.lib()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    scene, cam, cfg = scenes.build_config(key)
    fresh, _, _ = scenes.build_config(key)   # the second scene object: rebuilt at the new vertices
    W, H = cfg["W"], cfg["H"]
    n = scene.instance_count()
    _, blas_meshes = mesh_table(scene)
    counts = blas_counts(scene, len(blas_meshes))
    per_blas = np.bincount([scene.instance_info(i)["blas"] for i in range(n)], minlength=len(blas_meshes))
    b = int(np.argmax([c["prims"] for c in counts])) if key == "C5" else int(np.argmax(per_blas))
    mesh_id = blas_meshes[b][0]
    V0, N0, vi, ni = scene.mesh_arrays(mesh_id)
    uvt = texcoords(scene, mesh_id)
    note("%s: two scenes built, %d instances; BLAS %d (%d instances, %d triangles), mesh %d (%d vertices%s)"
         % (key, n, b, per_blas[b], counts[b]["prims"], mesh_id, len(V0), ", texture coordinates" if uvt else ""))
    Va, Vb = moved(V0, 1), moved(V0, 2)
    fresh_mesh = mesh_table(fresh)[0][mesh_id]   # given arrays: its vertices can change between builds

    def fresh_at(V):
        fresh_mesh.path, fresh_mesh.ctm = None, None
        fresh_mesh.setArrays(V, N0, vi, ni)
        if uvt:
            fresh_mesh.setTexCoords(*uvt)
        fresh.preCalc()
        _lib.check(L.mrt_scene_upload(fresh.handle, 0), "upload")

    rgb = torch.empty(H * W * 3, dtype=torch.float32, device=dev)
    cc = cam._c()
    opts = _lib.mrt_render_opts(W, H, 0, 0, 0, 0, 0)

    def render(s):
        _lib.check(L.mrt_render_frame_async(s.handle, C.byref(cc), C.byref(opts), rgb.data_ptr(), None, stream), "frame")

    def settle(ss):
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < SETTLE_S:
            for s in ss:
                render(s)
            torch.cuda.synchronize()

    _lib.check(L.mrt_scene_upload(scene.handle, 0), "upload")
    render(scene)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    render(scene)
    torch.cuda.synchronize()
    between = time.perf_counter() - t0 < 0.1   # a frame between the timed deforms, where it is cheap

    def after():
        if between:
            render(scene)
            torch.cuda.synchronize()

    scene.deformMesh(mesh_id, Va)   # the first refit of a replica makes its schedule: not timed
    settle([scene])
    refit, wall = [], []
    for r in range(rounds):
        v = Vb if r % 2 == 0 else Va
        t0 = time.perf_counter()
        ms = scene.deformMesh(mesh_id, v)
        wall.append((time.perf_counter() - t0) * 1e3)
        refit.append(ms)
        after()
    asyn = None
    if not uvt:
        ta, tb = torch.from_numpy(Va).to(dev), torch.from_numpy(Vb).to(dev)
        torch.cuda.synchronize()
        asyn = []
        for r in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            scene.deformMesh(mesh_id, tb if r % 2 == 0 else ta)
            e1.record()
            e1.synchronize()
            asyn.append(e0.elapsed_time(e1))
            after()
    note("%s: deform timed" % key)
    rebuild, world, blas_ms = [], [], []
    for r in range(max(2, rounds // 3)):   # the route before this entry (the frame after it is not timed)
        t0 = time.perf_counter()
        fresh_at(Vb if r % 2 == 0 else Va)
        torch.cuda.synchronize()
        rebuild.append((time.perf_counter() - t0) * 1e3)
        world.append(fresh.bvh_build_ms)
        blas_ms.append(fresh.blas_build_ms)
        if between:
            render(fresh)
            torch.cuda.synchronize()
    note("%s: rebuild route timed" % key)
    # frames: the refitted trees at Va against the fresh build at Va
    scene.deformMesh(mesh_id, Va)
    fresh_at(Va)
    img_r, img_f = miro.Image(), miro.Image()
    img_r.resize(W, H); img_f.resize(W, H)
    hr = scene.raytraceImage(cam, img_r, want_hits=True)
    hf = fresh.raytraceImage(cam, img_f, want_hits=True)
    agree = (hr["prim"] == hf["prim"]) & (hr["t"].view(np.uint32) == hf["t"].view(np.uint32))
    note("%s: hits compared" % key)
    settle([scene, fresh])
    frames = {"refit": [], "fresh": []}
    for q in range(frame_rounds):
        note("%s: frames, round %d of %d" % (key, q + 1, frame_rounds))
        for name, s in (("refit", scene), ("fresh", fresh)):
            render(s)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(frame_reps):
                render(s)
            e1.record()
            e1.synchronize()
            frames[name].append(e0.elapsed_time(e1) / frame_reps)
    info = scene.bvh_info
    blas_heights = heights(scene.blas_export(b)[1])
    world_heights = heights(scene.bvh_export()[1])
    out = {"scene": key, "instances": n, "world_prims": info["prims"], "world_nodes": info["nodes"], "world_leaves": info["leaves"],
           "world_heights": world_heights, "blas": b, "blas_instances": int(per_blas[b]), "blas_prims": counts[b]["prims"],
           "blas_nodes": counts[b]["nodes"], "blas_leaves": counts[b]["leaves"], "blas_heights": blas_heights,
           "mesh": mesh_id, "mesh_vertices": len(V0), "textured": bool(uvt),
           # scatter, BLAS leaf + node kernels, instance boxes, world leaf + node kernels
           "launches": 1 + 1 + blas_heights + 1 + 1 + world_heights,
           "W": W, "H": H, "rounds": rounds, "frame_rounds": frame_rounds, "frame_reps": frame_reps,
           "frame_between_deforms": bool(between), "library": _lib.build_info(L)["library"],
           "refit_ms": med(refit), "refit_wall_ms": med(wall), "refit_async_ms": med(asyn) if asyn else None,
           "rebuild_upload_ms": med(rebuild), "world_build_ms": med(world), "blas_build_ms": med(blas_ms),
           "frame_refit_ms": med(frames["refit"]), "frame_fresh_ms": med(frames["fresh"]),
           "hits_agree": round(float(agree.mean()), 6)}
    out["rebuild_over_refit_wall"] = round(out["rebuild_upload_ms"]["median"] / out["refit_wall_ms"]["median"], 1)
    out["frame_refit_over_fresh"] = round(out["frame_refit_ms"]["median"] / out["frame_fresh_ms"]["median"], 4)
    return out


def main():
    if miro.device_count() < 1:
        raise SystemExit("deform_bench.py: no HIP device visible (timings need the GPU)")
    keys = [a for a in sys.argv[1:] if a in ("C5", "FS")] or ["C5", "FS"]
    rounds = opt("--rounds", 9)
    frame_rounds, frame_reps = opt("--frame-rounds", rounds), opt("--frame-reps", FRAME_REPS)
    path = opt("--out", os.path.join(ROOT, "profiles", "deform_bench.json"))
    results = []
    if os.path.exists(path) and "--append" in sys.argv:
        with open(path) as f:
            results = [r for r in json.load(f) if r["scene"] not in keys]
    for key in keys:
        results.append(measure(key, rounds, frame_rounds, frame_reps))
        print(json.dumps(results[-1]), flush=True)
        with open(path, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
