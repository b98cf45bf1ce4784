"""Shading caller-supplied hits against shading caller rays: what does mrt_shade_hits_async cost
next to mrt_sample_rays_async on the same rays?  (One process, one device; needs the GPU.)

    python tools/shade_hits_ab.py [C3 R3 ...] [--rounds R] [--reps K] [--out FILE]

Per config, at its own frame size, with device buffers throughout, on the camera's own rays
(mrt_camera_rays) in image layout (row_width = W):
  rays     mrt_sample_rays_async: primary rays, then shading
  shade    mrt_shade_hits_async on the hits mrt_trace_rays_async found: the conversion of the
           records (20 B read, 16 B written per ray) in the primary launch's place, then shading
  trace    mrt_trace_rays_async alone (closest hits, the rays' times)
  surfaces mrt_hit_surfaces_async on those hits
The variants alternate within each round after a clock-settle period and a warm-up of each; a
sample is the HIP-event time of K back-to-back calls on one stream, divided by K.  Before
timing, the traced hits and the shaded frame are compared with mrt_sample_rays' bit for bit.
Prints one JSON line per config; --out appends them to a file.  (tools/sample_rays_ab.py is
the model.)"""
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


def measure(key, rounds, reps):
    L = miro.lib()
    scene, cam, cfg = scenes.build_config(key)
    W, H = cfg["W"], cfg["H"]
    n = W * H
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    o, d, t = (torch.from_numpy(x).to(dev) for x in cam.rays(W, H))
    lo = torch.full((n,), 0.001, dtype=torch.float32, device=dev)
    hi = torch.full((n,), 1e12, dtype=torch.float32, device=dev)
    ref = torch.empty(n * 3, dtype=torch.float32, device=dev)
    out = torch.empty(n * 3, dtype=torch.float32, device=dev)
    ref_hits = torch.empty((n, 5), dtype=torch.int32, device=dev)
    hits = torch.empty((n, 5), dtype=torch.int32, device=dev)
    surf = torch.empty((n, 21), dtype=torch.int32, device=dev)
    h = scene.handle

    def rays(want_hits=False):
        _lib.check(L.mrt_sample_rays_async(h, o.data_ptr(), d.data_ptr(), t.data_ptr(), n, W, 0, 0, ref.data_ptr(),
                                           ref_hits.data_ptr() if want_hits else None, stream), "sample_rays")

    def trace():
        _lib.check(L.mrt_trace_rays_async(h, o.data_ptr(), d.data_ptr(), t.data_ptr(), lo.data_ptr(), hi.data_ptr(), n, 0,
                                          hits.data_ptr(), stream), "trace_rays")

    def shade():
        _lib.check(L.mrt_shade_hits_async(h, o.data_ptr(), d.data_ptr(), t.data_ptr(), hits.data_ptr(), n, W, 0, 0,
                                          out.data_ptr(), stream), "shade_hits")

    def surfaces():
        _lib.check(L.mrt_hit_surfaces_async(h, o.data_ptr(), d.data_ptr(), hits.data_ptr(), n, surf.data_ptr(), stream),
                   "hit_surfaces")

    variants = {"rays": rays, "shade": shade, "trace": trace, "surfaces": surfaces}
    # same bits first (also the warm-up of every variant's kernels and scratch)
    _lib.check(L.mrt_scene_upload(h, 0), "upload")
    rays(True)
    trace()
    shade()
    stats = scene.stats()
    surfaces()
    assert torch.equal(hits, ref_hits), "traced hits differ from the sampled records"
    assert np.array_equal(out.cpu().numpy().view(np.uint32), ref.cpu().numpy().view(np.uint32)), "shaded frame differs"
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
    return {"config": key, "W": W, "H": H, "rays": n, "rounds": rounds, "reps": reps,
            "library": _lib.build_info(L)["library"], "chain": stats["chain"], "ms": m,
            "shade_over_rays": round(m["shade"]["median"] / m["rays"]["median"], 4),
            "trace_plus_shade_over_rays": round((m["trace"]["median"] + m["shade"]["median"]) / m["rays"]["median"], 4),
            # the conversion's traffic: one 20-B record read and one 16-B record written per ray
            "convert_MB": round(n * 36 / 1e6, 2)}


def main():
    if miro.device_count() < 1:
        raise SystemExit("shade_hits_ab.py: no HIP device visible (timings need the GPU)")
    keys = [a for a in sys.argv[1:] if a in scenes.CONFIGS] or ["C3", "R3"]
    rounds, reps, path = opt("--rounds", 9), opt("--reps", 10), opt("--out", "")
    for key in keys:
        line = json.dumps(measure(key, rounds, reps))
        print(line, flush=True)
        if path:
            with open(path, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
