// mrt_rebuild.h -- internal: the rule of mrt_scene_rebuild_bvh as functions the
// host (rebuild_host, host_build.cpp) and the kernels (mrt_rebuild.hip) share: the Morton key of
// a lane, the binary radix tree over the packet keys (Karras 2012) and which of its nodes root a
// 4-wide node.  tests/test_rebuild.py restates the rule in numpy without them.
#pragma once
#include <stdint.h>

#include "mrt_math.h"

namespace mrt {

// one axis of a lane's centre in the root box [rlo, rhi], 10 bits: separately rounded single ops
MRT_HD uint32_t rb_quant(float lo, float hi, float rlo, float rhi) {
    const float c = 0.5f * (lo + hi);
    const float e = rhi - rlo;
    const float t = (c - rlo) / e * 1024.0f;
    if (!(e > 0.f) || !(t >= 0.f)) return 0u;
    return t < 1023.f ? (uint32_t)(int)t : 1023u;
}
// bit i of a 10-bit value to bit 3 i
MRT_HD uint32_t rb_spread(uint32_t v) {
    v &= 1023u;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
// 30-bit Morton code (x, y, z per triple, most significant triple first) over the lane's position
MRT_HD uint64_t rb_key(const float lo[3], const float hi[3], const float rlo[3], const float rhi[3], uint32_t pos) {
    const uint32_t m = (rb_spread(rb_quant(lo[0], hi[0], rlo[0], rhi[0])) << 2) |
                       (rb_spread(rb_quant(lo[1], hi[1], rlo[1], rhi[1])) << 1) |
                       rb_spread(rb_quant(lo[2], hi[2], rlo[2], rhi[2]));
    return ((uint64_t)m << 32) | pos;
}

MRT_HD int rb_clz64(uint64_t x) {   // x != 0: the keys are unique
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)x);
#else
    return __builtin_clzll(x);
#endif
}
// delta(i, j): common prefix of keys i and j, -1 out of range
MRT_HD int rb_delta(const uint64_t* keys, int64_t n, int64_t i, int64_t j) {
    return j < 0 || j >= n ? -1 : rb_clz64(keys[i] ^ keys[j]);
}
// the digit of a binary node over keys first .. last: two bit levels make one 4-wide level
MRT_HD int rb_digit(const uint64_t* keys, int64_t first, int64_t last) { return rb_clz64(keys[first] ^ keys[last]) >> 1; }

// Binary node i (0 .. n - 2) of the radix tree over n >= 2 sorted unique keys: its range
// first .. last and its split g (left child g, right child g + 1).
MRT_HD void rb_karras(const uint64_t* keys, int64_t n, int64_t i, int64_t& first, int64_t& last, int64_t& g) {
    const int64_t d = rb_delta(keys, n, i, i + 1) - rb_delta(keys, n, i, i - 1) < 0 ? -1 : 1;
    const int dmin = rb_delta(keys, n, i, i - d);
    int64_t lmax = 2;
    while (rb_delta(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
    int64_t l = 0;
    for (int64_t t = lmax / 2; t >= 1; t /= 2)
        if (rb_delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
    const int64_t j = i + l * d;
    const int dn = rb_delta(keys, n, i, j);
    int64_t s = 0;
    for (int64_t t = (l + 1) / 2;; t = (t + 1) / 2) {
        if (rb_delta(keys, n, i, i + (s + t) * d) > dn) s += t;
        if (t <= 1) break;
    }
    g = i + s * d + (d < 0 ? -1 : 0);
    first = d > 0 ? i : j;
    last = d > 0 ? j : i;
}
// a child of the split as a word: >= 0 a binary node, ~p packet p
MRT_HD int32_t rb_left(int64_t first, int64_t g) { return first == g ? ~(int32_t)g : (int32_t)g; }
MRT_HD int32_t rb_right(int64_t last, int64_t g) { return last == g + 1 ? ~(int32_t)(g + 1) : (int32_t)(g + 1); }

// The children of the 4-wide node binary node b roots, in key order: b's two children, one
// that is a binary node of b's digit replaced by its own two (two levels at most: the prefix
// grows by a bit per level).  first / last / left / right: the binary nodes' arrays.
MRT_HD int rb_children(const uint64_t* keys, const int32_t* first, const int32_t* last, const int32_t* left,
                       const int32_t* right, int32_t b, int32_t out[4]) {
    const int dg = rb_digit(keys, first[b], last[b]);
    const int32_t two[2] = {left[b], right[b]};
    int n = 0;
    for (int k = 0; k < 2; k++) {
        const int32_t c = two[k];
        if (c >= 0 && rb_digit(keys, first[c], last[c]) == dg) {
            out[n++] = left[c];
            out[n++] = right[c];
        } else {
            out[n++] = c;
        }
    }
    return n;
}

}  // namespace mrt
