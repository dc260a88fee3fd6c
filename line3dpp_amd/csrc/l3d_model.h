// l3d_model.h -- the sizes and the slicing that the stages on a flat model of 3D segments share (DESIGN §16-§19:
// project, associate, compare, merge; their host plumbing is l3d_model.hip, declared in l3d_ctx.h), and the bounding box
// and the Cholesky solve of the stages that iterate about a model's centre (§23, §27-§29).  Plain C++17 without a HIP
// include (g++ compiles it for tests/test_model_slicing.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>

namespace l3d {

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }   // device tables start at multiples of 256 bytes
// Offsets of tables packed one behind the other: take() hands out the next 256-aligned offset and moves behind the
// table, so that `at` is the size of everything taken so far.
struct Layout {
    size_t at = 0;
    size_t take(size_t bytes) { const size_t o = up256(at); at = o + bytes; return o; }
};

constexpr uint32_t kSliceChunk = 256;    // references per chunk (= kCmpChunk of l3d_kernels.h)
// Slices of a walk of n_queries queries over n_refs references (both > 0), and the chunks per slice that go with them:
// a workgroup per (tile of queries, slice), bytes_per_cell bytes of partial results per (query, slice), which stay
// within budget -- fewer, longer slices where they would not.  The library's own choice (asked_chunks = 0) is ONE CHUNK
// PER SLICE: measured on C1 and C2 it is the fastest of the slicings tried or level with it, where a rule
// that aims at 1024 workgroups was 35 % slower at C2 (13 slices of 5 chunks on 65 tiles: 3.3 workgroups per compute
// unit, where seven fit).  No slice is empty and every chunk is covered, which the kernels rely on.
struct SlicePlan { uint32_t n_slices, slice_chunks; };
inline SlicePlan slice_plan(uint32_t n_queries, uint32_t n_refs, uint32_t asked_chunks, size_t bytes_per_cell, size_t budget) {
    const uint32_t n_chunks = (n_refs + kSliceChunk - 1) / kSliceChunk;
    const size_t cells = budget / (bytes_per_cell * (size_t)n_queries);
    const uint32_t cap = cells < 1 ? 1u : cells > n_chunks ? n_chunks : (uint32_t)cells;
    SlicePlan p;
    p.slice_chunks = asked_chunks ? (asked_chunks < n_chunks ? asked_chunks : n_chunks) : 1;
    p.n_slices = (n_chunks + p.slice_chunks - 1) / p.slice_chunks;
    if (p.n_slices <= cap) return p;
    p.slice_chunks = (n_chunks + cap - 1) / cap;
    p.n_slices = (n_chunks + p.slice_chunks - 1) / p.slice_chunks;
    return p;
}

// midpoint c and diagonal of the bounding box of the n > 0 segments' end points (the centre about which the
// alignment, the pose refinement, the refit and the bundle work)
inline void bounding_box(size_t n, const double* segs, double c[3], double& diag) {
    double lo[3] = {segs[0], segs[1], segs[2]}, hi[3] = {segs[0], segs[1], segs[2]};
    for (size_t i = 0; i < 2 * n; ++i)
        for (int k = 0; k < 3; ++k) {
            const double v = segs[3 * i + k];
            if (v < lo[k]) lo[k] = v;
            if (v > hi[k]) hi[k] = v;
        }
    double e[3];
    for (int k = 0; k < 3; ++k) { c[k] = (lo[k] + hi[k]) * 0.5; e[k] = hi[k] - lo[k]; }
    diag = std::sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
}

// H x = rhs for a symmetric H of n rows, of which the upper triangle H[i * n + j], i <= j, is read, by a plain Cholesky
// factorisation H = L L^T, column by column, then the forward and the backward substitution: the loops DESIGN §23 writes
// out, which the alignment (n = 6 or 7), the pose refinement of §27 (n = 6) and the reduced camera system of §29 share.
// work: n * (n + 1) doubles of the caller's -- kCholeskyWork on the stack for n <= kCholeskyMax, the heap beyond; x may be
// rhs.  false: a pivot that is not finite and > 0, x untouched.
constexpr size_t kCholeskyMax = 7, kCholeskyWork = kCholeskyMax * (kCholeskyMax + 1);
inline bool cholesky_solve(size_t n, const double* H, const double* rhs, double* x, double* work) {
    double* L = work;            // [n x n], the lower triangle
    double* y = work + n * n;
    for (size_t j = 0; j < n; ++j) {
        double p = H[j * n + j];
        for (size_t k = 0; k < j; ++k) p = p - L[j * n + k] * L[j * n + k];
        if (!(p > 0.0) || !std::isfinite(p)) return false;
        L[j * n + j] = std::sqrt(p);
        for (size_t i = j + 1; i < n; ++i) {
            double v = H[j * n + i];
            for (size_t k = 0; k < j; ++k) v = v - L[i * n + k] * L[j * n + k];
            L[i * n + j] = v / L[j * n + j];
        }
    }
    for (size_t i = 0; i < n; ++i) {
        double v = rhs[i];
        for (size_t k = 0; k < i; ++k) v = v - L[i * n + k] * y[k];
        y[i] = v / L[i * n + i];
    }
    for (size_t i = n; i-- > 0;) {
        double v = y[i];
        for (size_t k = i + 1; k < n; ++k) v = v - L[k * n + i] * x[k];
        x[i] = v / L[i * n + i];
    }
    return true;
}

}  // namespace l3d
