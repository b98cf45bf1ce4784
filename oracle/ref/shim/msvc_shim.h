/* Force-included ahead of every translation unit of the reference build
 * (oracle/ref/Makefile): the MSVC spellings its sources use, in g++ terms.
 * Our own text; nothing here comes from the reference. */
#ifndef MRT_REF_MSVC_SHIM_H
#define MRT_REF_MSVC_SHIM_H

#include <math.h>
#include <cmath>
#undef INFINITY              /* the reference declares a constant of that name */
#include <stdlib.h>
#include <string.h>
#include <float.h>
#include <stdio.h>
#include <xmmintrin.h>
#include <smmintrin.h>
#include <algorithm>
#include <iostream>
#include <vector>
#include <memory>
#include <string>
#include <omp.h>

#define __forceinline inline __attribute__((always_inline))
#define _MM_ALIGN16 __attribute__((aligned(16)))
#define __declspec(x) __attribute__((x))
#define align(n) aligned(n)

static inline void* _aligned_malloc(size_t size, size_t alignment) {
    void* p = 0;
    if (alignment < sizeof(void*)) alignment = sizeof(void*);
    return posix_memalign(&p, alignment, size ? size : alignment) == 0 ? p : 0;
}
static inline void _aligned_free(void* p) { free(p); }

#endif
