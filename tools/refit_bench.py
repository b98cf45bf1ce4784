"""Refit against rebuild: what does mrt_scene_update_mesh cost next to the only route there was
before it, mrt_scene_build_bvh + mrt_scene_upload?  (One process, one device; needs the GPU.)

    python tools/refit_bench.py [C3L BUDDHA ...] [--rounds R] [--out FILE]

Scenes: C3L (the 262 k-triangle Sponza stand-in, its config's camera and light) and BUDDHA (the
1.09 M-triangle buddha stand-in as a plain world mesh under a point light).  Per scene, after
a clock-settle period of untimed frames, medians over R rounds of
  rebuild_upload_ms  wall time of mrt_scene_build_bvh + mrt_scene_upload (measured first, on the
                     scene as built: nothing to read back)
  refit_ms           device events around the refit kernels of the synchronous entry (scatter,
                     leaf kernel, one node kernel per height)
  refit_wall_ms      wall time of the synchronous mrt_scene_update_mesh (copy in, kernels, wait)
  refit_async_ms     device events around mrt_scene_update_mesh_async on device tensors
the updates alternating between two displaced vertex sets; then, at one moderate displacement,
  frame_refit_ms / frame_fresh_ms   device time of a frame (mrt_render_frame_async, K back to
                     back) on the refitted tree and on a fresh build at the same vertices,
                     alternating
the share of pixels whose hit (prim, t) agrees between the two trees, and whether the arrays
the device holds after the refit equal the host's refit of the same scene.  Writes a JSON list
(default profiles/refit_bench.json) and prints one line per scene."""
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
FRAME_REPS = 10


def opt(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def displaced(V, seed, amp):
    """V + a smooth seeded displacement of amplitude `amp` (scene units) along each axis."""
    rng = np.random.default_rng(seed)
    ext = V.max(0) - V.min(0)
    d = np.stack([np.sin(V @ (rng.uniform(2, 6, 3) / ext) * 2 * np.pi + rng.uniform(0, 6.28)) for _ in range(3)], -1)
    return np.ascontiguousarray(V + amp * d, np.float32)


def build(key, verts=None):
    """(scene, camera, W, H) with the mesh to update as mesh 0 (vertices replaced by `verts`)."""
    if key == "C3L":
        cfg = scenes.CONFIGS["C3L"]
        if verts is None:
            scene, cam, _ = scenes.build_config("C3L")
            return scene, cam, cfg["W"], cfg["H"]
        src, _, _ = scenes.build_config("C3L")
        _, N, F, NI = src.mesh_arrays(0)
        mat, light_cfg, cam_cfg, bg = scenes.make_material(cfg["material"]), cfg["lights"][0], cfg["camera"], cfg["bg"]
    else:
        cfg = None
        V0, F, N = scenes.buddha_full_standin()
        verts = np.ascontiguousarray(V0 if verts is None else verts, np.float32)
        NI = F
        mat = miro.Blinn((0.8, 0.7, 0.6))
        light_cfg, bg = dict(pos=(2.0, 6.0, 5.0), power=300.0), (0.0, 0.0, 0.2)
        cam_cfg = dict(eye=(0.3, 1.5, 3.6), lookAt=(0.0, 1.2, 0.0), up=(0, 1, 0), fov=45.0)
    scene = miro.Scene()
    tm = miro.TriangleMesh()
    tm.setArrays(verts, N, F, NI)
    miro.makeMeshObjs(scene, tm, mat)
    pl = miro.PointLight()
    pl.setPosition(light_cfg["pos"])
    pl.setPower(light_cfg["power"])
    scene.addLight(pl)
    scene.setBGColor(bg)
    scene.preCalc()
    cam = miro.Camera()
    cam.setEye(cam_cfg["eye"]); cam.setLookAt(cam_cfg["lookAt"]); cam.setUp(cam_cfg["up"]); cam.setFOV(cam_cfg["fov"])
    return scene, cam, 1920, 1080


def med(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def measure(key, rounds):
    L = miro.lib()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    scene, cam, W, H = build(key)
    h = scene.handle
    V0, N0, _, _ = scene.mesh_arrays(0)
    amp = 0.01 * float((V0.max(0) - V0.min(0)).max())   # a moderate displacement: 1% of the mesh's extent
    Va, Vb = displaced(V0, 1, amp), displaced(V0, 2, amp)
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

    _lib.check(L.mrt_scene_upload(h, 0), "upload")
    render(scene)
    torch.cuda.synchronize()
    settle([scene])
    rebuild, build_ms = [], []
    for _ in range(max(3, rounds // 3)):   # the route before this entry: build + upload (the frame after it is not timed)
        t0 = time.perf_counter()
        _lib.check(L.mrt_scene_build_bvh(h), "build")
        t1 = time.perf_counter()
        _lib.check(L.mrt_scene_upload(h, 0), "upload")
        torch.cuda.synchronize()
        rebuild.append((time.perf_counter() - t0) * 1e3)
        build_ms.append((t1 - t0) * 1e3)
        render(scene)
        torch.cuda.synchronize()
    scene.updateMesh(0, Va)   # the first refit of a replica makes its schedule: not timed
    settle([scene])
    refit, wall = [], []
    for r in range(rounds):
        v = Vb if r % 2 == 0 else Va
        t0 = time.perf_counter()
        ms = scene.updateMesh(0, v)
        wall.append((time.perf_counter() - t0) * 1e3)
        refit.append(ms)
        render(scene)
        torch.cuda.synchronize()
    ta, tb = torch.from_numpy(Va).to(dev), torch.from_numpy(Vb).to(dev)
    torch.cuda.synchronize()
    asyn = []
    for r in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        scene.updateMesh(0, tb if r % 2 == 0 else ta)
        e1.record()
        e1.synchronize()
        asyn.append(e0.elapsed_time(e1))
        render(scene)
        torch.cuda.synchronize()
    # frames: the refitted tree at Va against a fresh build at Va
    scene.updateMesh(0, Va)
    # at this size: the arrays the device holds against the same refit done on the host (a scene never uploaded)
    host, _, _, _ = build(key)
    host.updateMesh(0, Va)
    arrays_equal = all(bool(np.array_equal(a, b)) for a, b in zip(scene.bvh_export(), host.bvh_export()))
    del host
    fresh, _, _, _ = build(key, Va)
    _lib.check(L.mrt_scene_upload(fresh.handle, 0), "upload")
    img_r, img_f = miro.Image(), miro.Image()
    img_r.resize(W, H); img_f.resize(W, H)
    hr = scene.raytraceImage(cam, img_r, want_hits=True)
    hf = fresh.raytraceImage(cam, img_f, want_hits=True)
    agree = (hr["prim"] == hf["prim"]) & (hr["t"].view(np.uint32) == hf["t"].view(np.uint32))
    same_rgb = bool(np.array_equal(img_r.rgb.view(np.uint32)[agree], img_f.rgb.view(np.uint32)[agree]))
    settle([scene, fresh])
    frames = {"refit": [], "fresh": []}
    for _ in range(rounds):
        for name, s in (("refit", scene), ("fresh", fresh)):
            render(s)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(FRAME_REPS):
                render(s)
            e1.record()
            e1.synchronize()
            frames[name].append(e0.elapsed_time(e1) / FRAME_REPS)
    info = scene.bvh_info
    out = {"scene": key, "triangles": info["prims"], "nodes": info["nodes"], "leaves": info["leaves"],
           "node_launches": info["max_depth"], "W": W, "H": H, "rounds": rounds, "displacement": round(amp, 5),
           "library": _lib.build_info(L)["library"],
           "rebuild_upload_ms": med(rebuild), "build_ms": med(build_ms), "refit_ms": med(refit), "refit_wall_ms": med(wall),
           "refit_async_ms": med(asyn), "frame_refit_ms": med(frames["refit"]), "frame_fresh_ms": med(frames["fresh"]),
           "hits_agree": round(float(agree.mean()), 6), "agreeing_pixels_same_rgb": same_rgb,
           "device_arrays_equal_host_refit": arrays_equal}
    out["rebuild_over_refit_wall"] = round(out["rebuild_upload_ms"]["median"] / out["refit_wall_ms"]["median"], 1)
    out["frame_refit_over_fresh"] = round(out["frame_refit_ms"]["median"] / out["frame_fresh_ms"]["median"], 4)
    return out


def main():
    if miro.device_count() < 1:
        raise SystemExit("refit_bench.py: no HIP device visible (timings need the GPU)")
    keys = [a for a in sys.argv[1:] if a in ("C3L", "BUDDHA")] or ["C3L", "BUDDHA"]
    rounds = opt("--rounds", 9)
    path = opt("--out", os.path.join(ROOT, "profiles", "refit_bench.json"))
    results = []
    for key in keys:
        results.append(measure(key, rounds))
        print(json.dumps(results[-1]), flush=True)
        with open(path, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
