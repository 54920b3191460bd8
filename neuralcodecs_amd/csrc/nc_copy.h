// The one device body every table-driven copy and overlap-add is made of (ragged batches, sessions, the session pool, the Encodec
// stream pool): a destination run is split at its first 16-byte boundary -- scalar head, whole 16-byte
// stores, scalar tail -- and stored exactly over [0, total), at any alignment of the destination and of whatever it is made from.
#pragma once
#include <algorithm>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace nc {

// blocks of 256 threads, one 16-byte vector per thread and round, at most 4096 blocks along x
inline unsigned copy_grid_x(int64_t longest, size_t elt) {
    const int64_t per_block = 256 * (16 / (int64_t)elt);
    return (unsigned)std::min<int64_t>(std::max<int64_t>(1, (longest + per_block - 1) / per_block), 4096);
}

#ifdef __HIPCC__
template <class T>
struct alignas(16) Vec16 { T v[16 / sizeof(T)]; };

// d[i] = at(i) for i in [0, total), nothing else is written.  blockIdx.x strides over the run: consecutive lanes store consecutive
// vectors.  vec_at(i) names V = 16 / sizeof(T) consecutive source elements equal to at(i) .. at(i + V - 1), or null where there is no
// such piece; where it is 16-byte aligned the vector is one load, otherwise the elements come from at().
template <class T, class At, class VecAt>
__device__ __forceinline__ void store_split16(T* d, int64_t total, At at, VecAt vec_at) {
    constexpr int V = 16 / sizeof(T);
    const int64_t mis = (int64_t)((reinterpret_cast<uintptr_t>(d) & 15) / sizeof(T));
    const int64_t head = mis ? (total < V - mis ? total : V - mis) : 0;
    const int64_t nvec = (total - head) / V, tail0 = head + nvec * V;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    if (tid < head) d[tid] = at(tid);
    for (int64_t v = tid; v < nvec; v += stride) {
        const int64_t base = head + v * V;
        const T* p = vec_at(base);
        Vec16<T> x;
        if (p && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            x = *reinterpret_cast<const Vec16<T>*>(p);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) x.v[j] = at(base + j);
        }
        *reinterpret_cast<Vec16<T>*>(d + base) = x;
    }
    if (tid < total - tail0) d[tail0 + tid] = at(tail0 + tid);
}
// computed elements: no source to load a vector from
template <class T, class At>
__device__ __forceinline__ void store_split16(T* d, int64_t total, At at) {
    store_split16<T>(d, total, at, [](int64_t) { return static_cast<const T*>(nullptr); });
}

// element i of a[0, na) ++ b[0, nb) ++ zeros
template <class T>
__device__ __forceinline__ T cat_at(const T* __restrict__ a, int64_t na, const T* __restrict__ b, int64_t nb, int64_t i) {
    return i < na ? a[i] : (i < na + nb ? b[i - na] : T(0));
}

// d[j] = (a ++ b ++ zeros)[s0 + j] for j in [0, total): reads stay inside a[0, na) and b[0, nb), writes inside d[0, total).
// Aliasing.  Callers pass the same buffer as a piece and as the destination (pool_assemble_body's `hist`, the stream gather's carry,
// the stream overlap-add's frames): a launch never reads an element that it writes -- a slot's current half is only read, its other
// half only written -- and `__restrict__` here says that and no more.
template <class T>
__device__ __forceinline__ void concat_copy(const T* __restrict__ a, int64_t na, const T* __restrict__ b, int64_t nb, int64_t s0,
                                            T* __restrict__ d, int64_t total) {
    constexpr int V = 16 / sizeof(T);
    store_split16<T>(
        d, total, [=](int64_t j) { return cat_at(a, na, b, nb, s0 + j); },
        [=](int64_t j) -> const T* {   // the vector lies inside one of the two pieces
            const int64_t i = s0 + j;
            if (i + V <= na) return a + i;
            if (i >= na && i + V <= na + nb) return b + (i - na);
            return nullptr;
        });
}
#endif

}  // namespace nc
