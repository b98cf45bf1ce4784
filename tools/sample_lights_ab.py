"""Sampling the lights at caller points against shading the same points as hits: what does
mrt_sample_lights_async cost next to mrt_shade_hits_async?  (One process, one device; needs the GPU.)

    python tools/sample_lights_ab.py [C3 C4 C5 ...] [--rounds R] [--reps K] [--out FILE]

Per config, at its own frame size, with device buffers throughout, on a twin of the config whose
materials are all white Lambert (kd = 1, ka = 0) with one path -- the one scene on which the two
entries compute the same numbers, so the older one can stand in for the new one:
  shade   mrt_shade_hits_async on the camera's own rays (mrt_camera_rays, row_width = W) and
          the closest hits mrt_trace_rays_async found: the records' conversion, then the
          shading dispatch (the wavefront passes -- gen, binned shadow rays, resolve -- or the
          one-light kernel)
  lights  mrt_sample_lights_async on the points and normals mrt_hit_surfaces_async gives for
          those hits: one fused kernel, a lane per point, nothing binned
Before timing, `e` is compared with the shaded frame bit for bit on every hit row (a miss row
holds the background there and a zero point here), and the shadow-ray counts are printed.
The variants alternate within each round after a clock-settle period and a warm-up of each; a
sample is the HIP-event time of K back-to-back calls on one stream, divided by K.  Prints one
JSON line per config; --out appends them to a file.  (tools/shade_hits_ab.py is the model.)"""
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


def opt(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def white_twin(key):
    """The config with every material a white Lambert and one path."""
    twin = "_white_" + key
    scenes.CONFIGS[twin] = dict(scenes.CONFIGS[key], material=dict(kind="lambert", kd=(1, 1, 1)), num_paths=1)
    try:
        return scenes.build_config(twin)
    finally:
        del scenes.CONFIGS[twin]


def measure(key, rounds, reps):
    L = miro.lib()
    scene, cam, cfg = white_twin(key)
    W, H = cfg["W"], cfg["H"]
    n = W * H
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    o, d, t = (torch.from_numpy(x).to(dev) for x in cam.rays(W, H))
    lo = torch.full((n,), 0.001, dtype=torch.float32, device=dev)
    hi = torch.full((n,), 1e12, dtype=torch.float32, device=dev)
    hits = torch.empty((n, 5), dtype=torch.int32, device=dev)
    surf = torch.empty((n, 21), dtype=torch.int32, device=dev)
    rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
    e = torch.empty((n, 3), dtype=torch.float32, device=dev)
    h = scene.handle
    _lib.check(L.mrt_scene_upload(h, 0), "upload")
    _lib.check(L.mrt_trace_rays_async(h, o.data_ptr(), d.data_ptr(), t.data_ptr(), lo.data_ptr(), hi.data_ptr(), n, 0,
                                      hits.data_ptr(), stream), "trace_rays")
    _lib.check(L.mrt_hit_surfaces_async(h, o.data_ptr(), d.data_ptr(), hits.data_ptr(), n, surf.data_ptr(), stream),
               "hit_surfaces")
    words = surf.view(torch.float32)   # mrt_surface: p at words 0-2, n at 3-5
    p, nrm = words[:, 0:3].contiguous(), words[:, 3:6].contiguous()

    def shade():
        _lib.check(L.mrt_shade_hits_async(h, o.data_ptr(), d.data_ptr(), t.data_ptr(), hits.data_ptr(), n, W, 0, 0,
                                          rgb.data_ptr(), stream), "shade_hits")

    def lights():
        _lib.check(L.mrt_sample_lights_async(h, p.data_ptr(), nrm.data_ptr(), None, t.data_ptr(), n, 0, 0, 0, 0,
                                             e.data_ptr(), None, stream), "sample_lights")

    variants = {"shade": shade, "lights": lights}
    # same bits first (also the warm-up of both variants' kernels and scratch)
    shade()
    shade_stats = scene.stats()
    lights()
    light_stats = scene.stats()
    hit = (hits[:, 3] >= 0).cpu().numpy()
    a, b = e.cpu().numpy().view(np.uint32)[hit], rgb.cpu().numpy().view(np.uint32)[hit]
    assert np.array_equal(a, b), "e differs from the shaded frame on %d of %d hit rows" % ((a != b).any(1).sum(), len(a))
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < SETTLE_S:   # clock settle: untimed work
        for f in variants.values():
            f()
        torch.cuda.synchronize()
    samples = {k: [] for k in variants}
    for _ in range(rounds):
        for name, f in variants.items():
            f()   # this variant's warm-up after the previous one
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            e1.synchronize()
            samples[name].append(e0.elapsed_time(e1) / reps)
    m = {k: {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
         for k, v in samples.items()}
    return {"config": key, "twin": "white Lambert, 1 path", "W": W, "H": H, "points": n, "hit_rows": int(hit.sum()),
            "rounds": rounds, "reps": reps, "library": _lib.build_info(L)["library"], "ms": m,
            "shadow_rays": {"shade": int(shade_stats["shadow_rays"]), "lights": int(light_stats["shadow_rays"])},
            "lights_over_shade": round(m["lights"]["median"] / m["shade"]["median"], 4)}


def main():
    if miro.device_count() < 1:
        raise SystemExit("sample_lights_ab.py: no HIP device visible (timings need the GPU)")
    keys = [a for a in sys.argv[1:] if a in scenes.CONFIGS] or ["C3", "C4", "C5"]
    rounds, reps, path = opt("--rounds", 9), opt("--reps", 10), opt("--out", "")
    for key in keys:
        line = json.dumps(measure(key, rounds, reps))
        print(line, flush=True)
        if path:
            with open(path, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
