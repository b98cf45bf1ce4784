"""The reference's float libm calls (atan2f / acosf of the lat-long lookups,
src/Texture.cpp:82-93; sinf(acosf(c)) of Fresnel, src/Material.h:51; cosf / sinf of the
cosine sampler, src/Material.cpp:41; powf of Blinn's specular lobe, src/Blinn.cpp:219)
against the device's restatements of glibc 2.35 (csrc/mrt_libm.h: fdlibm atan2f / acosf;
the optimized-routines sinf / cosf / powf of the x86-64 FMA build).

CPU: the restatements, compiled for the host with the device's flags (-ffp-contract=off;
the FMA build's contractions are explicit fma() calls), equal the host libm on every one
of the 2^32 acosf, sinf and cosf inputs, on 2^24 seeded atan2f pairs plus the special
values, and on powf over 2^22 seeded pairs, the special values and every float in [0, 1]
for the specular exponents of the scenes.  GPU: the same functions on the device
(the mrt_debug_libm probe) equal the oracle's glibc calls on 2^22 inputs each."""
import os
import subprocess

import numpy as np
import pytest

import miro
import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rendering-algorithms-raytracer_amd", "csrc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("libm") / "libm_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I", CSRC,
                           os.path.join(HERE, "native", "libm_check.cpp"), "-o", exe, "-lm"])
    return exe


def test_acosf_all_inputs(harness):
    """acosf over all 2^32 bit patterns, in 8 ranges run side by side."""
    step = 1 << 29
    procs = [subprocess.Popen([harness, "acos", str(lo), str(lo + step)], stdout=subprocess.PIPE, text=True)
             for lo in range(0, 1 << 32, step)]
    outs = [p.communicate()[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
    assert sum(int(o.split()[1]) for o in outs) == 1 << 32


@pytest.mark.parametrize("fn", ["sin", "cos"])
def test_sincosf_all_inputs(harness, fn):
    """sinf / cosf over all 2^32 bit patterns (every reduction branch: the polynomial
    below pi / 4, reduce_fast below 120, reduce_large above), 8 ranges side by side."""
    step = 1 << 29
    procs = [subprocess.Popen([harness, fn, str(lo), str(lo + step)], stdout=subprocess.PIPE, text=True)
             for lo in range(0, 1 << 32, step)]
    outs = [p.communicate()[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
    assert sum(int(o.split()[1]) for o in outs) == 1 << 32


def test_powf_pairs(harness):
    out = subprocess.run([harness, "pow", str(1 << 22), "4242"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout


def test_powf_unit_interval(harness):
    """powf(x, e) for every float in [0, 1] (the lobe's base, r.l clamped at 0) and the
    specular exponents the scenes use, 8 ranges side by side."""
    hi = 0x3F800001
    step = -(-hi // 8)
    procs = [subprocess.Popen([harness, "powx", str(lo), str(min(hi, lo + step)), "2", "8", "10", "32"],
                              stdout=subprocess.PIPE, text=True) for lo in range(0, hi, step)]
    outs = [p.communicate()[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o


def test_atan2f_pairs(harness):
    out = subprocess.run([harness, "atan2", str(1 << 24), "12345"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout


def test_probe_argument_checks_come_before_any_device_call():
    """mrt_debug_libm: fn out of range, a null x or out, a null y for the two-argument
    functions (1 atan2, 5 pow) -- MRT_ERR_INVALID, on a host without a device too."""
    L = miro.lib()
    buf = np.zeros(4, np.float32)
    p = buf.ctypes.data
    for fn, x, y, out in ((-1, p, p, p), (6, p, p, p), (0, None, p, p), (0, p, p, None), (1, p, None, p),
                          (5, p, None, p)):
        assert L.mrt_debug_libm(fn, x, y, 4, out) == -1, (fn, x, y, out)
        assert L.mrt_last_error().decode() == "bad libm probe arguments"
    if miro.device_count() < 1:   # one argument: y is not needed; the next stop is the device
        assert L.mrt_debug_libm(0, p, None, 4, p) == -7


@pytest.mark.gpu
@pytest.mark.parametrize("fn", ["acos", "atan2", "sin", "cos", "pow"])
def test_device_libm_equals_glibc(fn):
    if miro.device_count() < 1:
        pytest.skip("no HIP device")
    rng = np.random.default_rng(7)
    n = 1 << 22
    if fn == "acos":   # every 2^10-th bit pattern of [-1, 1], then random floats in [-1.1, 1.1]
        pos = np.arange(0, 0x3F800001, 1024, dtype=np.uint32)
        x = np.concatenate([pos.view(np.float32), (pos | 0x80000000).view(np.float32),
                            rng.uniform(-1.1, 1.1, n).astype(np.float32)])
        y = np.zeros_like(x)
    elif fn in ("sin", "cos"):   # every 2^10-th bit pattern (both signs, every branch), then [0, 2 pi)
        pos = np.arange(0, 0x7F800000, 1024, dtype=np.uint32)
        x = np.concatenate([pos.view(np.float32), (pos | 0x80000000).view(np.float32),
                            (2 * np.pi * rng.random(n)).astype(np.float32)])
        y = np.zeros_like(x)
    elif fn == "pow":   # the lobe's domain (x in [0, 1], the scenes' exponents), then seeded pairs
        xs = rng.random(n).astype(np.float32)
        es = rng.choice(np.array([2, 8, 10, 32, 1.5, 100], np.float32), n)
        u = rng.integers(0, 1 << 32, size=(2, n), dtype=np.uint64).astype(np.uint32)
        x = np.concatenate([xs, u[0].view(np.float32)])
        y = np.concatenate([es, u[1].view(np.float32)])
    else:
        u = rng.integers(0, 1 << 32, size=(2, n), dtype=np.uint64).astype(np.uint32)
        y, x = u[0].view(np.float32), u[1].view(np.float32)
        y = np.concatenate([y, rng.standard_normal(n).astype(np.float32)])
        x = np.concatenate([x, rng.standard_normal(n).astype(np.float32)])
    got = miro.debug_libm(fn, x, y)
    ref = O.libm_eval(fn, x, y)
    same = (got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref))
    assert same.all(), f"{fn}: {int((~same).sum())} of {len(x)} differ"
